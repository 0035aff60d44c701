#!/usr/bin/env python3
"""Cold ADMM, warm ADMM (dekf_set_warm_start), the direct solve (dekf_set_solver(h, DEKF_SOLVER_DIRECT)), the direct solve with the
window smoother (dekf_set_smoother; mode direct_smooth) and that with the window cross-covariances (dekf_set_window_cross; mode
direct_cross) on the four BASELINE shapes: Go1 B=4096, Cassie B=4096, PogoX B=1024 (N = 100)
and Go1 with foot-position states (leg_odom_type 1) B=4096.  One JSON line per shape, the modes side by side, each with
  steps_per_s   over `steps` timed steps after the window has filled (device-resident logs, the loop of tools/warm_start_bench.py)
  solve_ms      average launch time of the MHE solve (timing class 2, HIP events), in a second pass over the same steps
  assemble_ms   average launch time of the term construction (timing class 1: k_mhe_assemble), same pass
  kernel        the full-window solve kernel
and appends them to profiles/r08_direct_bench.jsonl, to profiles/r09_smoother_bench.jsonl when direct_smooth is among the modes, or to
profiles/r10_cross_bench.jsonl when direct_cross is (--out).  Timing class 1 and 2 events are only on in the second pass, so
steps_per_s is measured without them.  --repeat R measures the modes R times in turn (direct, direct_smooth, direct_cross, direct,
direct_smooth, direct_cross, ...) and reports each mode's best steps_per_s and lowest solve_ms with the list of all of them: the modes
alternate inside one process, so that a drift of the machine does not land on one of them.
    python tools/direct_bench.py [shape ...] [--steps 200] [--modes cold,warm,direct] [--repeat 1] [--out FILE]
    python tools/direct_bench.py --modes direct,direct_smooth --repeat 3          # the smoother against its yardstick
    python tools/direct_bench.py --modes direct,direct_smooth,direct_cross --repeat 3   # the cross-covariances against theirs
    python tools/direct_bench.py go1 cassie pogox --modes direct,direct_innov --repeat 3   # the innovation statistics (dekf_set_innovation;
                                                     # profiles/r10_innovation_bench.jsonl; not for go1_foot: outside the interface)
    python tools/direct_bench.py go1 cassie pogox --modes direct,direct_innov,direct_innov_gate --repeat 3   # the innovation gate
                                                     # (dekf_set_innovation_gate; profiles/r11_gate_bench.jsonl).  The log then carries a
                                                     # few foot slips (every 512th robot, three ticks) and the bound is high, so the
                                                     # common path is "decide, gate nothing"; gated_last: legs gated at the last step
    python tools/direct_bench.py go1 cassie pogox --modes direct_smooth_innov,direct_smooth_innov_gate_window --repeat 3
                                                     # the window of a gating handle (dekf_set_gate_smoother;
                                                     # profiles/r15_gate_smoother_bench.jsonl): the smoother with the innovation kernel
                                                     # against the same with the gate kernel's _smooth twin, on the slip-carrying log.
                                                     # --gate-bound 150 prices the gated path itself; gated_total: legs gated over the
                                                     # timed steps
--epoch measures what dekf_reset_instances costs the instances it does not restart: per mode ONE handle runs the unchanged direct
kernel (`before`), then restarts instance 0, lets its window refill and runs the epoch twins (`after`); dekf_reset brings the handle
back, and the two alternate --repeat times in one process.  One JSON line per shape (--out: profiles/r11_epoch_bench.jsonl).
    python tools/direct_bench.py go1 --epoch --modes direct,direct_smooth,direct_cross --steps 80 --repeat 3
--instance-params measures what a parameter table (dekf_set_instance_params) costs: per mode ONE handle runs the unchanged direct
kernels (`before`: no table), then, after dekf_reset, the _pp twins with B distinct sets (`after`), and the two alternate --repeat
times in one process.  One JSON line per shape (--out: profiles/r12_instance_params_bench.jsonl).
    python tools/direct_bench.py go1 --instance-params --modes direct,direct_smooth,direct_cross --repeat 3
--epoch --paused F[,F...] measures what dekf_set_active costs and saves: per mode ONE handle restarts instance 0 and runs the epoch
twins with every instance active (`ep`, the yardstick), then for every fraction F pauses that share of the batch, spread evenly over
it (0: one instance paused and resumed in the same gap, so the handle launches the *_act kernels with nobody paused), and runs again
(`paused_F`); dekf_reset brings the handle back, and the runs alternate --repeat times in one process.  One JSON line per shape
(--out: profiles/r13_pause_bench.jsonl).
    python tools/direct_bench.py go1 --epoch --paused 0,0.5,0.9 --modes direct,direct_smooth,direct_cross --steps 80 --repeat 3
--snapshot measures dekf_save_instances and dekf_load_instances: per mode ONE handle runs past its window fill, then saves all B
instances to a device blob and loads them back into their own slots, --repeat times, each call between two events on the handle's
stream; beside them one device-to-device hipMemcpyAsync of the blob's byte count on the same stream, the yardstick the two kernels are
read against.  One JSON line per shape (--out: profiles/r14_snapshot_bench.jsonl).
    python tools/direct_bench.py go1 --snapshot --modes direct_smooth --repeat 5"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from decentralized_ekf_mhe_amd import cassie_params, go1_params, pogox_params  # noqa: E402
from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_to_device  # noqa: E402
from decentralized_ekf_mhe_amd.streams import make_streams  # noqa: E402

SHAPES = {
    "go1": (go1_params, 4096, {}),
    "cassie": (cassie_params, 4096, {}),
    "pogox": (pogox_params, 1024, {}),
    "go1_foot": (go1_params, 4096, {"leg_odom_type": 1}),
}
MODES = {"cold": dict(), "warm": dict(warm_start=True), "direct": dict(solver="direct"),
         "direct_smooth": dict(solver="direct", smoother=True), "direct_cross": dict(solver="direct", smoother=True, cross=True),
         "direct_innov": dict(solver="direct", innovation=True),
         "direct_innov_gate": dict(solver="direct", innovation=True, innovation_gate=1e4),
         "direct_smooth_innov": dict(solver="direct", smoother=True, innovation=True),
         "direct_smooth_innov_gate_window": dict(solver="direct", innovation=True, innovation_gate=1e4, gate_smoother=True)}
GATE_MODES = ("direct_innov_gate", "direct_smooth_innov_gate_window")
GATE_SLIP = (-12.8, 8.0, -5.4)   # m/s, IMU frame: far above the bound on every shape (nis_leg of 4e4 and more)


def add_slips(s, W, steps):
    """foot slips on the first stance leg of every 512th robot at three ticks of the timed steps, the last step among them"""
    import numpy as np
    for k in (W + steps // 3, W + 2 * steps // 3, W + steps - 1):
        for b in range(0, s["contact"].shape[1], 512):
            legs = np.nonzero(s["contact"][k, b])[0]
            if len(legs):
                s["qdot"][k, b, legs[0]] += np.linalg.pinv(s["J"][k, b, legs[0]]) @ np.array(GATE_SLIP)
    return s


def one(p, B, sd, W, steps, mode):
    est = BatchedEstimator(p, B, **MODES[mode])
    for k in range(W):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(W, W + steps):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the same steps once more with events around the assemble and the solve launches (a handle's steps are not repeatable, so a second
    # handle replays the log: same inputs, same kernels)
    est2 = BatchedEstimator(p, B, **MODES[mode])
    for k in range(W):
        est2.push_stream_step(sd, k)
        est2.step(k)
    est2.sync()
    est2.timing_enable(1)
    gated_total = 0
    for k in range(W, W + steps):
        est2.push_stream_step(sd, k)
        est2.step(k)
        if mode in GATE_MODES:  # (a read between the steps of the pass that is timed by events around the launches alone)
            gated_total += int(est2.innovation_gate()[1].sum())
    tim = est2.timing_read()
    solved = float((est2.get()["status"] == 1).mean())
    kernel = est.solve_kernel_name(True)
    gated = {"gated_last": int(est2.innovation_gate()[1].sum()), "gated_total": gated_total,
             "gate_bound": MODES[mode]["innovation_gate"]} if mode in GATE_MODES else {}
    est.close()
    est2.close()
    return {"steps_per_s": B * steps / dt, "solve_ms": tim["solve"][0] / max(tim["solve"][1], 1),
            "assemble_ms": tim["assemble"][0] / max(tim["assemble"][1], 1), "ekf_ms": tim["ekf"][0] / max(tim["ekf"][1], 1),
            "solved_fraction": solved, "kernel": kernel, **gated}


def timed(est, sd, k0, steps, B):
    """`steps` steps from tick k0 without events, then `steps` more with events around every launch: (steps/s, ms per launch by class)"""
    est.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(k0, k0 + steps):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    est.timing_enable(1)
    est.timing_read()
    for k in range(k0 + steps, k0 + 2 * steps):
        est.push_stream_step(sd, k)
        est.step(k)
    tim = est.timing_read()
    est.timing_enable(0)
    return {"steps_per_s": B * steps / dt, "kernel": est.solve_kernel_name(True),
            **{f"{c}_ms": tim[c][0] / max(tim[c][1], 1) for c in ("solve", "assemble", "ekf")}}


def epoch_ticks(p, steps):
    """(W, refill, log length) of epoch_runs: warm-up, the restarted instance's window fill, and everything"""
    W, refill = max(p.N + 10, 64), p.N + 10
    return W, refill, W + 2 * steps + refill + 2 * steps


def epoch_runs(p, B, sd, steps, mode, repeat):
    """before / after a first dekf_reset_instances on one handle, `repeat` times in turn (dekf_reset in between)"""
    import numpy as np
    W, refill, _ = epoch_ticks(p, steps)
    est = BatchedEstimator(p, B, **MODES[mode])
    mask = np.zeros(B, np.int32)
    mask[0] = 1
    before, after = [], []
    for _ in range(repeat):
        est.reset()
        for k in range(W):
            est.push_stream_step(sd, k)
            est.step(k)
        before.append(timed(est, sd, W, steps, B))
        k1 = W + 2 * steps
        est.reset_instances(mask)
        for k in range(k1, k1 + refill):
            est.push_stream_step(sd, k)
            est.step(k)
        assert int(est.instance_ticks()[0]) == refill - 1 >= p.N
        after.append(timed(est, sd, k1 + refill, steps, B))
        assert float((est.get()["status"] == 1).mean()) == 1.0
    est.close()

    def best(runs):
        out = dict(max(runs, key=lambda r: r["steps_per_s"]))
        for c in ("solve", "assemble", "ekf"):
            out[f"{c}_ms"] = min(r[f"{c}_ms"] for r in runs)
        out["all_steps_per_s"] = [r["steps_per_s"] for r in runs]
        out["all_solve_ms"] = [r["solve_ms"] for r in runs]
        return out
    b, a = best(before), best(after)
    return {"before": b, "after": a, "solve_ms_after_over_before": a["solve_ms"] / b["solve_ms"],
            "assemble_ms_after_over_before": a["assemble_ms"] / b["assemble_ms"], "ekf_ms_after_over_before": a["ekf_ms"] / b["ekf_ms"],
            "steps_per_s_after_over_before": a["steps_per_s"] / b["steps_per_s"]}


def pause_ticks(p, steps, fractions):
    """(W, refill, log length) of pause_runs"""
    W, refill = max(p.N + 10, 64), p.N + 10
    return W, refill, W + refill + 2 * steps * (1 + len(fractions))


def pause_runs(p, B, sd, steps, mode, repeat, fractions):
    """the epoch twins with every instance active, then with the fractions of the batch paused, on one handle, `repeat` times in turn"""
    import numpy as np
    W, refill, _ = pause_ticks(p, steps, fractions)
    est = BatchedEstimator(p, B, **MODES[mode])
    first = np.zeros(B, np.int32)
    first[0] = 1
    runs = {"ep": [], **{f"paused_{f:g}": [] for f in fractions}}
    for _ in range(repeat):
        est.reset()
        for k in range(W):
            est.push_stream_step(sd, k)
            est.step(k)
        est.reset_instances(first)
        for k in range(W, W + refill):
            est.push_stream_step(sd, k)
            est.step(k)
        k0 = W + refill
        runs["ep"].append(timed(est, sd, k0, steps, B))
        assert runs["ep"][-1]["kernel"].endswith("_ep") and int(est.active().sum()) == B
        for f in fractions:
            k0 += 2 * steps
            b = np.arange(B)
            active = 1 - (np.floor((b + 1) * f) > np.floor(b * f)).astype(np.int32)
            if active.all():  # nobody paused: the *_act kernels all the same
                one_paused = np.ones(B, np.int32)
                one_paused[B // 2] = 0
                est.set_active(one_paused)
            est.set_active(active)
            r = timed(est, sd, k0, steps, B)
            r["paused"] = int(B - est.active().sum())
            runs[f"paused_{f:g}"].append(r)
            est.set_active(np.ones(B, np.int32))
        assert float((est.get()["status"] == 1).mean()) == 1.0

    def best(rs):
        out = dict(max(rs, key=lambda r: r["steps_per_s"]))
        for c in ("solve", "assemble", "ekf"):
            out[f"{c}_ms"] = min(r[f"{c}_ms"] for r in rs)
        out["all_steps_per_s"] = [r["steps_per_s"] for r in rs]
        out["all_solve_ms"] = [r["solve_ms"] for r in rs]
        return out
    est.close()
    out = {k: best(v) for k, v in runs.items()}
    for k in list(out):
        if k != "ep":
            out[k].update({f"{c}_over_ep": out[k][c] / out["ep"][c] for c in ("solve_ms", "assemble_ms", "ekf_ms", "steps_per_s")})
    return out


def snapshot_runs(p, B, sd, mode, repeat):
    """ms of saving all instances to a device blob, of loading them back, and of one device-to-device copy of as many bytes"""
    import numpy as np
    W = max(p.N + 10, 64)
    est = BatchedEstimator(p, B, **MODES[mode])
    for k in range(W):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    idx = np.arange(B, dtype=np.int32)
    stream = torch.cuda.ExternalStream(est.lib.dekf_stream(est.h))
    nbytes, per_instance = est.snapshot_bytes(B), est.snapshot_bytes(2) - est.snapshot_bytes(1)
    twin = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = {"save_ms": [], "load_ms": [], "memcpy_ms": []}

    def ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        r = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), r

    for _ in range(repeat + 1):   # (the first round is the warm-up: first launch of both kernels, first touch of both buffers)
        t_save, blob = ms(lambda: est.save_instances(idx, device=True))
        t_load, _ = ms(lambda: est.load_instances(idx, blob))
        with torch.cuda.stream(stream):
            t_copy, _ = ms(lambda: twin.copy_(blob, non_blocking=True))
        assert torch.equal(twin, blob)
        for key, v in (("save_ms", t_save), ("load_ms", t_load), ("memcpy_ms", t_copy)):
            out[key].append(v)
    for k in range(W, W + 4):     # the loaded handle goes on
        est.push_stream_step(sd, k)
        est.step(k)
    assert float((est.get()["status"] == 1).mean()) == 1.0 and est.solve_kernel_name(True).endswith("_ep")
    est.close()
    res = {"bytes": nbytes, "bytes_per_instance": per_instance}
    for key, v in out.items():
        v = v[1:]
        res[key] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}
    res["save_GB_per_s"] = nbytes / res["save_ms"]["median"] / 1e6
    res["load_GB_per_s"] = nbytes / res["load_ms"]["median"] / 1e6
    res["memcpy_GB_per_s"] = nbytes / res["memcpy_ms"]["median"] / 1e6
    return res


def distinct_sets(p, B):
    """B parameter sets, no two alike: every std of the noise fields scaled by a factor of its own in [0.8, 1.25]"""
    fields = ("p_init_std", "v_init_std", "foot_init_std", "accel_bias_init_std", "p_process_std", "accel_input_std", "gyro_input_std",
              "accel_bias_std", "joint_position_std", "joint_velocity_std", "foot_slide_std", "foot_swing_std", "vo_p_std", "ekf_init_std",
              "ekf_process_std", "ekf_gravity_meas_std", "ekf_vo_meas_std")
    sets = []
    for b in range(B):
        q = p.copy()
        for i, f in enumerate(fields):
            a = getattr(q, f)
            for j in range(len(a)):
                a[j] = a[j] * (0.8 + 0.45 * ((b * 7 + i * 3 + j) % B) / B)
        sets.append(q)
    return sets


def instance_params_runs(p, B, sd, steps, mode, repeat):
    """without / with a parameter table of B distinct sets on one handle, `repeat` times in turn (dekf_reset in between)"""
    import numpy as np
    W = max(p.N + 10, 64)
    est = BatchedEstimator(p, B, **MODES[mode])
    sets, set_of = distinct_sets(p, B), np.arange(B, dtype=np.int32)
    before, after = [], []
    for _ in range(repeat):
        for runs, table in ((before, False), (after, True)):
            est.reset()
            est.set_instance_params(sets if table else None, set_of if table else None)
            for k in range(W):
                est.push_stream_step(sd, k)
                est.step(k)
            runs.append(timed(est, sd, W, steps, B))
            assert runs[-1]["kernel"].endswith("_pp") == table
            assert float((est.get()["status"] == 1).mean()) == 1.0
    est.close()

    def best(runs):
        out = dict(max(runs, key=lambda r: r["steps_per_s"]))
        for c in ("solve", "assemble", "ekf"):
            out[f"{c}_ms"] = min(r[f"{c}_ms"] for r in runs)
        out["all_steps_per_s"] = [r["steps_per_s"] for r in runs]
        out["all_solve_ms"] = [r["solve_ms"] for r in runs]
        return out
    b, a = best(before), best(after)
    return {"before": b, "after": a, "solve_ms_after_over_before": a["solve_ms"] / b["solve_ms"],
            "assemble_ms_after_over_before": a["assemble_ms"] / b["assemble_ms"], "ekf_ms_after_over_before": a["ekf_ms"] / b["ekf_ms"],
            "steps_per_s_after_over_before": a["steps_per_s"] / b["steps_per_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--modes", default="cold,warm,direct")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--epoch", action="store_true", help="the same handle before and after a first dekf_reset_instances")
    ap.add_argument("--instance-params", action="store_true", help="the same handle without and with a table of B distinct parameter sets")
    ap.add_argument("--snapshot", action="store_true", help="dekf_save_instances / dekf_load_instances of the whole batch against a device-to-device copy")
    ap.add_argument("--gate-bound", type=float, default=None, help="the bound of the gating modes (default 1e4: almost nothing gates)")
    ap.add_argument("--paused", default=None, help="with --epoch: fractions of the batch to pause (dekf_set_active), e.g. 0,0.5,0.9")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if a.gate_bound is not None:
        for m in GATE_MODES:
            MODES[m]["innovation_gate"] = a.gate_bound
    fractions = [float(f) for f in a.paused.split(",")] if a.paused else []
    if fractions and not a.epoch:
        ap.error("--paused goes with --epoch")
    if a.out is None and a.snapshot:
        a.out = os.path.join(ROOT, "profiles", "r14_snapshot_bench.jsonl")
    if a.out is None and fractions:
        a.out = os.path.join(ROOT, "profiles", "r13_pause_bench.jsonl")
    if a.out is None and a.instance_params:
        a.out = os.path.join(ROOT, "profiles", "r12_instance_params_bench.jsonl")
    if a.out is None and a.epoch:
        a.out = os.path.join(ROOT, "profiles", "r11_epoch_bench.jsonl")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r15_gate_smoother_bench.jsonl" if "direct_smooth_innov_gate_window" in modes else
                             "r11_gate_bench.jsonl" if "direct_innov_gate" in modes else
                             "r10_innovation_bench.jsonl" if "direct_innov" in modes else
                             "r10_cross_bench.jsonl" if "direct_cross" in modes else
                             "r09_smoother_bench.jsonl" if "direct_smooth" in modes else "r08_direct_bench.jsonl")
    for name in a.shapes:
        maker, B, kw = SHAPES[name]
        p = maker()
        p.ekf_rate = p.rate
        for k, v in kw.items():
            setattr(p, k, v)
        if a.snapshot:
            sd = streams_to_device(make_streams(p, B, max(p.N + 10, 64) + 4))
            line = {"shape": name, "batch": B, "N": int(p.N), "repeat": a.repeat, "snapshot": True}
            line.update({mode: snapshot_runs(p, B, sd, mode, a.repeat) for mode in modes})
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del sd
            torch.cuda.empty_cache()
            continue
        if a.instance_params:
            sd = streams_to_device(make_streams(p, B, max(p.N + 10, 64) + 2 * a.steps))
            line = {"shape": name, "batch": B, "N": int(p.N), "steps": a.steps, "repeat": a.repeat, "instance_params": True}
            line.update({mode: instance_params_runs(p, B, sd, a.steps, mode, a.repeat) for mode in modes})
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del sd
            torch.cuda.empty_cache()
            continue
        if a.epoch and fractions:
            sd = streams_to_device(make_streams(p, B, pause_ticks(p, a.steps, fractions)[2]))
            line = {"shape": name, "batch": B, "N": int(p.N), "steps": a.steps, "repeat": a.repeat, "paused": fractions}
            line.update({mode: pause_runs(p, B, sd, a.steps, mode, a.repeat, fractions) for mode in modes})
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del sd
            torch.cuda.empty_cache()
            continue
        if a.epoch:
            sd = streams_to_device(make_streams(p, B, epoch_ticks(p, a.steps)[2]))
            line = {"shape": name, "batch": B, "N": int(p.N), "steps": a.steps, "repeat": a.repeat, "epoch": True}
            line.update({mode: epoch_runs(p, B, sd, a.steps, mode, a.repeat) for mode in modes})
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del sd
            torch.cuda.empty_cache()
            continue
        W = max(p.N + 10, 64)  # (as tools/bench_shapes.py: past the window fill and the first vision intervals)
        s = make_streams(p, B, W + a.steps)
        if any(m in modes for m in GATE_MODES + ("direct_smooth_innov",)):  # (every mode of the line runs the same log)
            s = add_slips(s, W, a.steps)
        sd = streams_to_device(s)
        line = {"shape": name, "batch": B, "N": int(p.N), "steps": a.steps}
        runs = {mode: [] for mode in modes}
        for _ in range(a.repeat):
            for mode in modes:
                runs[mode].append(one(p, B, sd, W, a.steps, mode))
        for mode in modes:
            best = dict(max(runs[mode], key=lambda r: r["steps_per_s"]))
            best["solve_ms"] = min(r["solve_ms"] for r in runs[mode])
            if a.repeat > 1:
                best["all_steps_per_s"] = [r["steps_per_s"] for r in runs[mode]]
                best["all_solve_ms"] = [r["solve_ms"] for r in runs[mode]]
            line[mode] = best
        if "direct" in line:
            line.update({f"direct_over_{m}": line["direct"]["steps_per_s"] / line[m]["steps_per_s"] for m in ("cold", "warm") if m in line})
        if "direct" in line and "direct_smooth" in line:
            line["smooth_solve_ms_over_direct"] = line["direct_smooth"]["solve_ms"] / line["direct"]["solve_ms"]
            line["smooth_steps_per_s_over_direct"] = line["direct_smooth"]["steps_per_s"] / line["direct"]["steps_per_s"]
        if "direct" in line and "direct_innov" in line:  # (timing class 2 brackets the solve and the innovation kernel as one launch)
            line["innov_solve_ms_over_direct"] = line["direct_innov"]["solve_ms"] / line["direct"]["solve_ms"]
            line["innov_steps_per_s_over_direct"] = line["direct_innov"]["steps_per_s"] / line["direct"]["steps_per_s"]
        if "direct_innov_gate" in line:
            for m, tag in (("direct", "direct"), ("direct_innov", "innov")):
                if m in line:
                    line[f"gate_solve_ms_over_{tag}"] = line["direct_innov_gate"]["solve_ms"] / line[m]["solve_ms"]
                    line[f"gate_steps_per_s_over_{tag}"] = line["direct_innov_gate"]["steps_per_s"] / line[m]["steps_per_s"]
        if "direct_smooth_innov_gate_window" in line and "direct_smooth_innov" in line:  # (class 2: the solve and the kernel behind it)
            line["gate_window_solve_ms_over_smooth_innov"] = line["direct_smooth_innov_gate_window"]["solve_ms"] / line["direct_smooth_innov"]["solve_ms"]
            line["gate_window_steps_per_s_over_smooth_innov"] = line["direct_smooth_innov_gate_window"]["steps_per_s"] / line["direct_smooth_innov"]["steps_per_s"]
        if "direct_cross" in line:
            for m, tag in (("direct", "direct"), ("direct_smooth", "smooth")):
                if m in line:
                    line[f"cross_solve_ms_over_{tag}"] = line["direct_cross"]["solve_ms"] / line[m]["solve_ms"]
                    line[f"cross_steps_per_s_over_{tag}"] = line["direct_cross"]["steps_per_s"] / line[m]["steps_per_s"]
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
