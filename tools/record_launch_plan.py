#!/usr/bin/env python3
"""Records tests/golden/launch_plan.json: the solve kernel names and grid of every configuration of tests/test_gpu_launch_plan.py
(its own list and its own observe()), with the device's compute units.  The fixture freezes what the library decides, so it is recorded
from the commit BEFORE a change to how a handle picks its kernel, never from the build under test.
    python tools/record_launch_plan.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import torch  # noqa: F401,E402  (torch's HIP runtime first: estimator._torch_runtime_first acts only when torch is already imported)
import test_gpu_launch_plan as LP  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else LP.GOLDEN
plans = {f"{name}/{B}": LP.observe(name, B) for name, B in LP.CASES}
with open(out, "w") as f:
    json.dump({"compute_units": LP.compute_units(), "plans": plans}, f, indent=1)
    f.write("\n")
print(f"{len(plans)} plans -> {out}")
