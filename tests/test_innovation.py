"""The innovation statistics of a direct handle (dekf_set_innovation / dekf_get_innovation, mhe_innov_core.h) without a GPU: the
lane-sequential build of the core against the oracle's window QP with the newest Meas rows made free, the identities the five arrays owe
each other, a poisoned sample, a stand-alone sanitizer program, the C boundary and the compiler's account of the eight kernels."""
import json
import os
import subprocess

import numpy as np
import pytest

import direct_lib as DL
import innov_lib as IL
from decentralized_ekf_mhe_amd import capi, go1_params

# what the checked ticks of a case must contain: a tick with every leg in flight, a tick with mixed contact, a window with VO equality rows
MUST_HOLD = {"go1": ("flight", "mixed", "vo"), "cassie": ("flight", "mixed", "vo"), "tripod": ("flight", "mixed", "vo"), "pogox": ("flight",)}


@pytest.mark.parametrize("name", list(IL.CPU_CASES))
def test_core_against_the_oracle_with_the_newest_meas_rows_free(name):
    """every checked tick of every instance within the limits of innov_lib (the worst figures are printed), the identities at every one
    of them, and the case holds the kinds of tick it is there for"""
    mk, B, K, ticks = IL.CPU_CASES[name]
    p, s, refs = IL.case_reference(name)
    got = IL.case_sim(name)
    worst, seen = {}, set()
    for b in range(B):
        for k in ticks:
            g, r = IL.instance(got[k], b), refs[b][k]
            assert got[k]["status"][b] == capi.DEKF_SOLVE_OK
            e = IL.errors(g, r)
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in e.items()}
            IL.assert_within_limits(e, (name, b, k))
            IL.check_identities(g, p.num_legs, (name, b, k))
            seen.add(IL.contact_kind(s, k, b))
            if r["vo"] > 0:
                seen.add("vo")
    print(name, {key: f"{v:.2e}" for key, v in worst.items()}, sorted(seen))
    assert set(MUST_HOLD[name]) <= seen, (MUST_HOLD[name], seen)


def test_flight_phase_figures():
    """in a flight phase every Q_m entry is 1e-14: NIS is of the order 1e-15 and log det S = -12 log(1e-14) = 386.8 (Go1), in the core
    as in the reference"""
    mk, B, K, ticks = IL.CPU_CASES["go1"]
    p, s, refs = IL.case_reference("go1")
    got = IL.case_sim("go1")
    flight = [(b, k) for b in range(B) for k in ticks if IL.contact_kind(s, k, b) == "flight"]
    assert flight
    for b, k in flight:
        g = IL.instance(got[k], b)
        assert 0.0 < g["nis"] < 1e-12 and abs(refs[b][k]["logdet"] - 386.83) < 0.01
        assert abs(-2.0 * g["loglik"] - g["nis"] - 12 * np.log(2 * np.pi) - refs[b][k]["logdet"]) < 1e-8


def test_one_leg_per_leg_nis_is_the_whole():
    """one leg: S is its own diagonal block, so nis_leg[0] = nis (two routes in the core: the inverse of W, and the LDL' of S)"""
    mk, B, K, ticks = IL.CPU_CASES["pogox"]
    p, s, _ = IL.case_reference("pogox")
    got = IL.case_sim("pogox")
    for k in ticks:
        g = IL.instance(got[k], 0)
        assert abs(g["nis_leg"].sum() - g["nis"]) <= 1e-12 * g["nis"], (k, g["nis_leg"], g["nis"])


def test_per_leg_nis_sums_to_the_whole_where_s_is_block_diagonal():
    """Go1 with one leg in stance and the others in flight: the flight legs' blocks of S are 1e14 against the stance leg's 1e-6 and the
    off-diagonal blocks H P^- H', so the scaled S is block diagonal to 1e-11 and the per-leg values sum to the whole to that"""
    mk, B, K, ticks = IL.CPU_CASES["go1"]
    p, s, _ = IL.case_reference("go1")
    got = IL.case_sim("go1")
    n = 0
    for b in range(B):
        for k in ticks:
            g = IL.instance(got[k], b)
            S = g["innov_cov"]
            d = 1.0 / np.sqrt(np.diagonal(S))
            Sn = S * d[:, None] * d[None, :]
            off = Sn.copy()
            for i in range(p.num_legs):
                off[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.0
            if np.abs(off).max() < 1e-9:
                n += 1
                assert abs(g["nis_leg"].sum() - g["nis"]) <= 1e-7 * g["nis"], (b, k)
    assert n >= 1


def test_a_nan_sample_poisons_one_instance_and_nobody_else():
    p = DL._params(go1_params)
    B, K, bad, t_bad = 3, 30, 1, 24
    s = DL.rough_streams(p, B, K)
    ticks = list(range(1, K))
    clean = IL.run_sim(p, s, B, K, ticks)
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan
    pois = IL.run_sim(p, sp, B, K, ticks)
    assert pois[t_bad]["status"][bad] == capi.DEKF_SOLVE_NUMERIC
    for k in ticks:
        for b in range(B):
            for key in IL.KEYS:
                if b != bad or k < t_bad:
                    assert np.isfinite(clean[k][key][b]).all()
                    assert np.array_equal(pois[k][key][b], clean[k][key][b]), (k, b, key)
                elif pois[k]["status"][bad] == capi.DEKF_SOLVE_NUMERIC:
                    assert np.isnan(pois[k][key][b]).all(), (k, key)


# ------------------------------------------------------------------ sanitizers
ASAN_BUFFERS = """    const int nm = 3 * L;
    std::vector<double> nu((size_t)B * nm, -7.0), S((size_t)B * nm * nm, -7.0), nis(B, -7.0), nl((size_t)B * L, -7.0), ll(B, -7.0);
"""
ASAN_UPDATE = """        if (hs_update_direct_innov(h, T, cov.data(), nu.data(), S.data(), nis.data(), nl.data(), ll.data())) return 3;
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < nm; ++i) bad += !std::isfinite(nu[(size_t)b * nm + i]);
            for (int i = 0; i < nm; ++i)
                for (int j = 0; j < nm; ++j) bad += !(S[((size_t)b * nm + i) * nm + j] == S[((size_t)b * nm + j) * nm + i]);
            for (int i = 0; i < L; ++i) bad += !(nl[(size_t)b * L + i] >= 0.0);
            bad += !(nis[b] >= 0.0) + !std::isfinite(ll[b]);
        }
"""
ASAN_REPORT = """    std::printf("nis %g loglik %g, %d bad entries\\n", nis[0], ll[0], bad);
"""


def test_core_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over innov_hostsim.cpp under AddressSanitizer + UBSan (CPU build, run directly): the core at L = 4, 2
    and 1, through the window fill, full windows and VO rows, with the contact pattern changing every five steps"""
    driver = DL.ASAN_DRIVER.replace('#include "direct_hostsim.cpp"', '#include "innov_hostsim.cpp"')
    main = "int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }"
    assert main in driver
    driver = driver.replace(main, "int main() { return run(4, 3, 20, 50, 0, 0) | run(2, 5, 6, 24, 0, 0) | run(1, 2, 30, 44, 0, 0); }")
    src = tmp_path / "innov_driver.cpp"
    src.write_text(driver.replace("//BUFFERS", ASAN_BUFFERS).replace("//UPDATE", ASAN_UPDATE).replace("//REPORT", ASAN_REPORT))
    exe = tmp_path / "innov_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", DL.HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 bad entries") == 3


# ------------------------------------------------------------------ the C boundary
SYMBOLS = ("dekf_set_innovation", "dekf_get_innovation")


def test_header_declares_both_calls_and_states_the_scope():
    hdr = DL.header()
    for name in SYMBOLS:
        assert f"dekf_status {name}(dekf_handle h" in hdr, name
    assert "leg_odom_type 1" in hdr[hdr.index("innovation statistics (opt-in"):] and "whole-window likelihoods" in hdr


def test_library_exports_and_binding_lists_them():
    DL.check_exports_and_binding(SYMBOLS)


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    assert lib.dekf_set_innovation(None, 1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_get_innovation(None, None, None, None, None, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID


def test_c99_client_calls_both_symbols(tmp_path):
    import torch
    body = ("    dekf_params p;\n    dekf_handle h = 0;\n    double nis[4];\n    dekf_default_params(&p);\n"
            "    int st = dekf_create(&p, 4, 0, 0, &h);\n"
            '    printf("create %d set %d get %d\\n", st, dekf_set_innovation(h, 1), dekf_get_innovation(h, 0, 0, nis, 0, 0, DEKF_HOST));\n'
            "    if (st == 0) dekf_destroy(h);\n")
    if torch.cuda.is_available():   # (an ADMM handle: the option is refused, the getter too)
        expect = f"create 0 set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID}"
    else:                           # no device, no handle: dekf_create still answers DEKF_ERR_NO_DEVICE
        expect = f"create {capi.DEKF_ERR_NO_DEVICE} set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID}"
    DL.check_c99_client(tmp_path, "innov_client", body, expect)


# ------------------------------------------------------------------ resource remarks
INNOV_USAGE = os.path.join(DL.CSRC, "libdekf_innov_resource_usage.txt")


def innov_usage_table():
    """the compiler's account of the innovation kernels' build unit (build.sh writes it beside libdekf_resource_usage.txt) by kernel
    name, and the static LDS by kernel name"""
    import re
    from test_resource_usage import _sources_mtime, parse_usage
    assert os.path.exists(INNOV_USAGE) and os.path.getmtime(INNOV_USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(INNOV_USAGE).read()
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    return parse_usage(text), static_lds


def test_the_eight_kernels_are_at_their_design_point():
    """no spills, no scratch, at most 72 VGPRs (the direct kernels' class), no static LDS"""
    table, static_lds = innov_usage_table()
    assert sorted(table) == sorted(IL.INNOV_KERNELS + ["k_innov_nan"])
    for n in IL.INNOV_KERNELS:
        u = table[n]
        print(n, u)
        assert u["spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0 and u["vgprs"] + (u["agprs"] or 0) <= IL.MAX_VGPRS, (n, u)
        assert static_lds[n] == 0, n


def test_the_kernels_of_before_keep_their_account():
    """libdekf_resource_usage.txt holds the kernels it held before this interface, each with the entry it had, and none of the new ones:
    those of tests/golden/resource_usage_before_pause.json and the six kernels of the pause interface (what tests/test_instance_pause.py
    asserts of that file).  The new kernels are a build unit of their own with a remarks file of their own"""
    table, _ = DL.usage_table()
    before = json.load(open(os.path.join(DL.ROOT, "tests", "golden", "resource_usage_before_pause.json")))
    assert all(table.get(k) == v for k, v in before.items())
    assert len(set(table) - set(before)) == 6 and not any(k.startswith(("k_mhe_innov", "k_innov")) for k in table)
