#!/usr/bin/env python3
"""One line per gfx950 kernel of a source tree: a hash of its instructions and the compiler's metadata entry.

    python tools/device_code_digest.py [--src TREE] [--jobs N] [--out FILE]

Host-only (no GPU).  Compiles TREE's kernels.hip once per unit of the product build (build.sh: -DDEKF_KSET=<mask> -DDEKF_KSET_ONLY,
masks 1 ... 512, 1024 ... 16384, with -mllvm -disable-machine-licm for the sets build.sh compiles without that pass) as device code
alone, disassembles every unit and prints, sorted by name,

    <symbol> <sha256 of the instruction encodings, addresses left out> <metadata fields>

Run it on two trees and diff the outputs: equal outputs mean that every kernel is instruction for instruction the same code with the
same kernarg size, register counts, spills, scratch and LDS.  (Hashes of the object files themselves differ between two directories.)
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

MASKS = [512, 256, 128, 64, 32, 16, 8, 4, 1, 2, 1024, 2048, 4096, 8192, 16384]  # heaviest first, as build.sh
NO_MLICM = {1, 2, 4, 64, 128, 256, 512}  # build.sh: DEKF_NO_MLICM's default
META = ["kernarg_segment_size", "vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size", "uses_dynamic_stack"]


def compile_unit(csrc, mask, tmp, rocm):
    obj = os.path.join(tmp, f"k_{mask}.o")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{rocm}/include", f"-I{csrc}"]
    if mask in NO_MLICM:
        cmd += ["-mllvm", "-disable-machine-licm"]
    cmd += ["--cuda-device-only", "--no-gpu-bundle-output", "-c", f"-DDEKF_KSET={mask}", "-DDEKF_KSET_ONLY", "-o", obj, "kernels.hip"]
    subprocess.run(cmd, cwd=csrc, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    llvm = os.path.join(rocm, "llvm", "bin")
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", obj], check=True, capture_output=True, text=True).stdout
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    return mask, code_hashes(dis), kernel_metadata(notes)


def code_hashes(dis):
    """symbol -> sha256 over the encoding words of its instructions (the text after '// <address>:', branch labels cut off)"""
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), hashlib.sha256())
            continue
        m = re.search(r"// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)", line)
        if m and cur is not None:
            cur.update(m.group(1).strip().encode() + b"\n")
    return {k: v.hexdigest()[:24] for k, v in out.items()}


def kernel_metadata(notes):
    """kernel name -> its fields of amdhsa.kernels (top-level scalars of every list entry)"""
    out, cur, inside = {}, None, False
    for line in notes.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):
            inside = False
            continue
        m = re.match(r"^(  - |    )\.([a-z_]+): +(\S.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
        if m.group(2) == "name":
            out[cur["name"]] = cur
    return out


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--src", default=here, help="the source tree (default: this one)")
    ap.add_argument("--jobs", type=int, default=min(len(MASKS), os.cpu_count() or 1))
    ap.add_argument("--out", default="-")
    ap.add_argument("--rocm", default=os.environ.get("ROCM_PATH", "/opt/rocm"))
    a = ap.parse_args()
    csrc = os.path.join(os.path.abspath(a.src), "decentralized_ekf_mhe_amd", "csrc")
    lines = []
    with tempfile.TemporaryDirectory(prefix="dekf_digest_") as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for mask, code, meta in pool.map(lambda m: compile_unit(csrc, m, tmp, a.rocm), MASKS):
            for sym in code:
                md = meta.get(sym)
                fields = " ".join(f"{k}={md.get(k, '-')}" for k in META) if md else "(not a kernel)"
                lines.append(f"{sym} set={mask} code={code[sym]} {fields}")
            missing = set(meta) - set(code)
            if missing:
                sys.exit(f"set {mask}: kernels in the metadata without code: {sorted(missing)}")
    text = "\n".join(sorted(lines)) + "\n"
    if a.out == "-":
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
