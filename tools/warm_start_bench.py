#!/usr/bin/env python3
"""Cold against warm start (dekf_set_warm_start) on the four BASELINE shapes: Go1 B=4096, Cassie B=4096, PogoX B=1024 (N = 100) and
Go1 with foot-position states (leg_odom_type 1) B=4096.  One JSON line per shape, cold and warm side by side:
  steps_per_s   over `steps` (>= 200) timed steps after the window has filled (device-resident logs, the loop of tools/bench_shapes.py)
  solve_ms      average launch time of the MHE solve (timing class 2, HIP events)
  iters         mean ADMM iterations and their histogram (fraction of solves), rho_updates the mean rho refactorisations, over
                `hist` further full-window ticks read one by one (a read synchronises: outside the timed region)
  warm_fraction of those solves that started warm (warm start on)
    python tools/warm_start_bench.py [shape ...] [--steps 200] [--hist 24]     shapes: go1 cassie pogox go1_foot (default: all)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def one(p, B, sd, W, steps, hist, warm):
    est = BatchedEstimator(p, B, warm_start=warm)
    for k in range(W):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    est.timing_enable(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(W, W + steps):
        est.push_stream_step(sd, k)
        est.step(k)
    est.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tim = est.timing_read()
    est.timing_enable(False)
    its, rhos, ws, sts = [], [], [], []
    for k in range(W + steps, W + steps + hist):
        est.push_stream_step(sd, k)
        est.step(k)
        info = est.solver_info()
        its.append(info["iters"].copy())
        rhos.append(info["rho_updates"].copy())
        ws.append(est.warm_status())
        sts.append(est.get()["status"])
    kernel = est.solve_kernel_name(True)
    est.close()
    its, rhos, ws, sts = (np.array(a) for a in (its, rhos, ws, sts))
    vals, cnt = np.unique(its, return_counts=True)
    return {"steps_per_s": B * steps / dt, "solve_ms": tim["solve"][0] / max(tim["solve"][1], 1), "solve_launches": tim["solve"][1],
            "iters_mean": float(its.mean()), "iters_hist": {int(v): round(float(c) / its.size, 4) for v, c in zip(vals, cnt)},
            "rho_updates_mean": float(rhos.mean()), "warm_fraction": float(ws.mean()), "solved_fraction": float((sts == 1).mean()),
            "kernel": kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--hist", type=int, default=24)
    a = ap.parse_args()
    for name in a.shapes:
        maker, B, kw = SHAPES[name]
        p = maker()
        p.ekf_rate = p.rate
        for k, v in kw.items():
            setattr(p, k, v)
        W = max(p.N + 10, 64)  # (as tools/bench_shapes.py: past the window fill and the first vision intervals)
        sd = streams_to_device(make_streams(p, B, W + a.steps + a.hist))
        cold = one(p, B, sd, W, a.steps, a.hist, False)
        warm = one(p, B, sd, W, a.steps, a.hist, True)
        print(json.dumps({"shape": name, "batch": B, "N": int(p.N), "steps": a.steps, "cold": cold, "warm": warm,
                          "speedup": warm["steps_per_s"] / cold["steps_per_s"]}), flush=True)
        del sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
