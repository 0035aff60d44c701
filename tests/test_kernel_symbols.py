"""No kernel is renamed or dropped: the kernels of the product build are the names of tests/golden/kernel_symbols.txt, and the direct
solve kernels among them are rows x variants of csrc/direct_kernels.def.

The names come from the compiler's resource remarks, which build.sh writes next to the library (libdekf_resource_usage.txt and, for
the innovation unit, libdekf_innov_resource_usage.txt).  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decentralized_ekf_mhe_amd", "csrc")
USAGE_FILES = ("libdekf_resource_usage.txt", "libdekf_innov_resource_usage.txt")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_symbols.txt")


def built_names():
    names = []
    newest_source = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".def", ".sh")))
    for f in USAGE_FILES:
        path = os.path.join(CSRC, f)
        assert os.path.exists(path), f"{f} is missing: run csrc/build.sh (the product build writes it)"
        assert os.path.getmtime(path) >= newest_source, f"{f} is older than the sources: run csrc/build.sh"
        names += re.findall(r"^Function Name: (\S+)$", open(path).read(), re.M)
    return names


def catalogue():
    """(rows, variant suffixes) of direct_kernels.def"""
    text = open(os.path.join(CSRC, "direct_kernels.def")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("//"))
    rows = sorted(set(re.findall(r"^DEKF_DIRECT_KERNEL\((\w+),", code, re.M)))
    off = sorted(set(re.findall(r"^DEKF_DIRECT_KERNEL_OFF\((\w+),", code, re.M)))
    assert rows == off, "every row has its expansion outside the kernel sets"
    suffixes = re.findall(r"^\s*V\((\w*),\s*[01],\s*[01],\s*(?:WINDOW|EPOCH|PARAM),", code, re.M)
    return rows, suffixes


def test_kernel_names_are_the_recorded_ones_and_the_direct_ones_are_rows_times_variants():
    names = built_names()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    recorded = open(FIXTURE).read().split()
    assert sorted(names) == recorded, {"missing": sorted(set(recorded) - set(names)), "new": sorted(set(names) - set(recorded))}

    rows, suffixes = catalogue()
    assert rows and suffixes and len(set(suffixes)) == len(suffixes), (rows, suffixes)
    direct = sorted(n for n in names if n.startswith("k_mhe_solve_direct_"))
    assert direct == sorted(r + s for r in rows for s in suffixes)
