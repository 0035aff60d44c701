"""The innovation gate of a direct handle (dekf_set_innovation_gate / dekf_get_innovation_gate, mhe_gate_core.h) without a GPU: the
reference's own decisions on logs with injected foot slips, the lane-sequential build of the core against that reference at two gates
per case, the record edit and the two bit contracts against a gate-off run on the edited log, a stand-alone sanitizer program, the C
boundary and the compiler's account of the eight kernels."""
import os
import subprocess

import numpy as np
import pytest

import direct_lib as DL
import gate_lib as GL
import innov_lib as IL
from decentralized_ekf_mhe_amd import capi

NAMES = list(GL.CASES)


def _stance_split(name, which):
    """(nominal, injected) reference nis_leg of the stance legs of a case: the injected pairs and all the others"""
    p, s, gate, ref = GL.case_reference(name, which)
    inj = set(GL.CASES[name][0])
    nom, hit = [], []
    for b, rb in ref.items():
        for k, r in rb.items():
            for leg in range(p.num_legs):
                if s["contact"][k, b, leg]:
                    (hit if (k, b, leg) in inj else nom).append(float(r["nis_leg"][leg]))
    return nom, hit


@pytest.mark.parametrize("name", NAMES)
def test_high_gate_reference_gates_exactly_the_injected_slips(name):
    """the high gate sits a factor 3 or more above the nominal maximum and below the injected minimum of the reference's nis_leg (both
    printed), the reference gates exactly the injected pairs, a swing leg never passes, and no nis_leg is within 1e-6 of the gate"""
    p, s, gate, ref = GL.case_reference(name, "high")
    nom, hit = _stance_split(name, "high")
    print(name, f"high gate {gate:g}: nominal stance nis_leg median {np.median(nom):.1f} p90 {np.percentile(nom, 90):.1f} max {max(nom):.1f}; "
          f"injected min {min(hit):.1f} max {max(hit):.1f}")
    assert 3.0 * max(nom) <= gate <= min(hit) / 3.0, (max(nom), gate, min(hit))
    assert GL.decisions(ref) == sorted(GL.CASES[name][0])
    GL.check_margin(ref, gate, name)
    swing = [r["nis_leg"][leg] for b, rb in ref.items() for k, r in rb.items() for leg in range(p.num_legs) if not s["contact"][k, b, leg]]
    assert max(swing) < 1e-9, max(swing)


def test_injected_slips_cover_what_they_are_there_for():
    """a window-fill tick, a full window, a window with VO equality rows, a tick with mixed contact, two legs of one robot at one tick
    and the only leg of the one-leg robot"""
    seen = set()
    for name in NAMES:
        p, s, gate, ref = GL.case_reference(name, "high")
        pairs = GL.CASES[name][0]
        for k, b, leg in pairs:
            seen.add("fill" if k + 1 < p.N else "full")
            if ref[b][k]["vo"] > 0:
                seen.add("vo")
            if IL.contact_kind(s, k, b) == "mixed":
                seen.add("mixed")
            if sum(1 for q in pairs if q[:2] == (k, b)) >= 2:
                seen.add("two legs")
            if p.num_legs == 1:
                seen.add("one-leg robot")
        if name != "pogox":
            assert {"fill", "full"} <= {("fill" if k + 1 < p.N else "full") for k, _, _ in pairs}, name
    assert seen == {"fill", "full", "vo", "mixed", "two legs", "one-leg robot"}, seen


@pytest.mark.parametrize("name", NAMES)
def test_low_gate_reference_shows_every_kind_of_tick(name):
    """the low gate sits inside the nominal spread: the reference then shows a tick with one gated leg, (robots with several legs) a tick
    with two or more, a tick where every stance leg of a robot is gated, and ungated ticks behind gated ones"""
    p, s, gate, ref = GL.case_reference(name, "low")
    nom, _ = _stance_split(name, "low")
    assert min(nom) < gate < max(nom), (min(nom), gate, max(nom))
    GL.check_margin(ref, gate, name)
    kinds = set()
    for b, rb in ref.items():
        was_gated = False
        for k in sorted(rb):
            n, stance = int(rb[k]["gated"].sum()), int(s["contact"][k, b].sum())
            assert (rb[k]["gated"] <= s["contact"][k, b]).all()
            if n == 1:
                kinds.add("one")
            if n >= 2:
                kinds.add("several")
            if n and n == stance:
                kinds.add("all stance legs")
            if not n and was_gated:
                kinds.add("ungated behind gated")
            was_gated = was_gated or n > 0
    print(name, f"low gate {gate:g}:", len(GL.decisions(ref)), "gated pairs", sorted(kinds))
    want = {"one", "all stance legs", "ungated behind gated"} | ({"several"} if p.num_legs > 1 else set())
    assert want <= kinds, (want, kinds)


@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_core_against_the_reference(name, which):
    """every tick of every instance: gated equal to the reference's decisions; the five arrays (those of the ungated problem) within
    innov_lib's limits; x_mhe within XREL / XABS and Cov(x_T) within CREL of the optimum of the QP with the gated blocks.  The worst
    errors are printed, those of the gated ticks apart"""
    p, s, gate, ref = GL.case_reference(name, which)
    run = GL.case_sim(name, which)
    worst = GL.check_against_reference(run, ref, list(ref), (name, which))
    print(name, which, {key: f"{v:.2e}" for key, v in sorted(worst.items())})
    assert any(key.startswith("gated ") for key in worst)


@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_record_block_and_bits_against_a_gate_off_run_on_the_edited_log(name, which):
    """a gate-off run fed the log with contact = 0 at the pairs an instance gated: at a gated tick the newest record's Q_m words are
    equal and the five arrays are those of the run that had not seen this tick's edit; at every tick at which the instance gates
    nothing, every output is equal to the bit; and v_b is the tail's function of x_mhe at a gated tick too (it agrees with the edited
    run's as x does)"""
    p, B, K, sub, s = GL.case_streams(name)
    _, _, gate, ref = GL.case_reference(name, which)
    run = GL.case_sim(name, which)
    dec = GL.decisions(ref)
    behind = GL.check_bits_on_ungated_ticks(run, lambda so, n: GL.run_sim(p, so, n, K), s, dec, B, K, (name, which))
    assert behind > 0
    for b in range(B):
        ticks, so = GL.edited_copies(s, b, B, dec)
        off = GL.run_sim(p, so, len(ticks) + 1, K)
        for i, k in enumerate(ticks):
            g = run[k - 1]
            # copy i + 1 has this tick's edit in its log, copy i has not
            assert np.array_equal(g["qm"][b], off[k - 1]["qm"][i + 1]), (name, b, k)
            assert not np.array_equal(g["qm"][b], off[k - 1]["qm"][i])
            for key in IL.KEYS:
                assert np.array_equal(g[key][b], off[k - 1][key][i]), (name, b, k, key)
            assert GL.x_err(g["x"][b], off[k - 1]["x"][i + 1]) <= 1.0 and DL.cov_err(g["cov"][b], off[k - 1]["cov"][i + 1]) <= DL.CREL
            # (v_b = R (v + w x p): a row of a rotation has a 1-norm of at most sqrt(3) < 2, so v_b moves by less than twice what v does)
            assert np.abs(g["v_b"][b] - off[k - 1]["v_b"][i + 1]).max() <= 2.0 * (DL.XREL * np.abs(off[k - 1]["x"][i + 1][3:6]).max() + DL.XABS)
            assert np.array_equal(g["cov"][b], g["cov"][b].T)


@pytest.mark.parametrize("name", NAMES)
def test_a_gate_that_never_fires_is_the_gate_off(name):
    never, off = GL.case_sim(name, "never"), GL.case_sim(name, "off")
    assert len(never) == len(off)
    for a, b in zip(never, off):
        assert not a["gated"].any()
        for key in GL.OUTPUTS + ("qm",):
            assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_a_failed_solve_gates_nothing():
    """NaN compares false: an instance whose solve failed (a poisoned sample) gates nothing, its neighbour gates what it gated"""
    p, B, K, sub, s = GL.case_streams("go1")
    gate = GL.CASES["go1"][2]
    clean = GL.run_sim(p, s, B, 30, gate)
    sp = GL.copy_streams(s)
    sp["accel"][24, 0, 0] = np.nan
    pois = GL.run_sim(p, sp, B, 30, gate)
    assert pois[23]["status"][0] == capi.DEKF_SOLVE_NUMERIC and not pois[23]["gated"][0].any() and np.isnan(pois[23]["nis_leg"][0]).all()
    for a, b in zip(clean, pois):
        assert np.array_equal(a["gated"][1], b["gated"][1]) and np.array_equal(a["x"][1], b["x"][1])


# ------------------------------------------------------------------ sanitizers
ASAN_BUFFERS = """    const int nm = 3 * L;
    std::vector<double> nu((size_t)B * nm, -7.0), S((size_t)B * nm * nm, -7.0), nis(B, -7.0), nl((size_t)B * L, -7.0), ll(B, -7.0);
    std::vector<int> gated((size_t)B * L, -7);
    int fired = 0;
"""
ASAN_UPDATE = """        // every seventh step a gate that every stance leg passes, else one that a leg passes now and then
        if (hs_update_direct_innov_gate(h, T, T % 7 == 3 ? 1e-3 : 40.0, cov.data(), nu.data(), S.data(), nis.data(), nl.data(), ll.data(), gated.data())) return 3;
        for (int b = 0; b < B; ++b) {
            int any = 0;
            for (int i = 0; i < L; ++i) {
                bad += gated[(size_t)b * L + i] != (nl[(size_t)b * L + i] > (T % 7 == 3 ? 1e-3 : 40.0) ? 1 : 0);
                any += gated[(size_t)b * L + i];
            }
            fired += any;
            for (int i = 0; i < ns; ++i)  // (the corrected covariance is symmetric to the bit, the direct solve's is finite)
                for (int j = 0; j < ns; ++j)
                    bad += any ? !(cov[((size_t)b * ns + i) * ns + j] == cov[((size_t)b * ns + j) * ns + i]) : !std::isfinite(cov[((size_t)b * ns + i) * ns + j]);
            bad += !(nis[b] >= 0.0) + !std::isfinite(ll[b]);
        }
"""
ASAN_REPORT = """    std::printf("%d legs gated, %d bad entries\\n", fired, bad);
    if (!fired) return 4;
"""


def test_gate_core_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over gate_hostsim.cpp under AddressSanitizer + UBSan (CPU build, run directly): the gate core on gated
    ticks of Go1 (L = 4), a two-leg robot and the one-leg case, through the window fill, full windows and VO rows"""
    driver = DL.ASAN_DRIVER.replace('#include "direct_hostsim.cpp"', '#include "gate_hostsim.cpp"')
    main = "int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }"
    assert main in driver
    driver = driver.replace(main, "int main() { return run(4, 3, 20, 50, 0, 0) | run(2, 5, 6, 24, 0, 0) | run(1, 2, 30, 44, 0, 0); }")
    src = tmp_path / "gate_driver.cpp"
    src.write_text(driver.replace("//BUFFERS", ASAN_BUFFERS).replace("//UPDATE", ASAN_UPDATE).replace("//REPORT", ASAN_REPORT))
    exe = tmp_path / "gate_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", DL.HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 bad entries") == 3


# ------------------------------------------------------------------ the C boundary
SYMBOLS = ("dekf_set_innovation_gate", "dekf_get_innovation_gate")


def test_header_declares_both_calls_and_states_the_scope():
    hdr = DL.header()
    for name in SYMBOLS:
        assert f"dekf_status {name}(dekf_handle h" in hdr, name
    text = hdr[hdr.index("innovation gate (opt-in"):]
    assert "the window of a gating handle is\n * not part of this interface" in text and "nis_leg[b][l] > nis_leg_max" in text


def test_library_exports_and_binding_lists_them():
    DL.check_exports_and_binding(SYMBOLS)


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    assert lib.dekf_set_innovation_gate(None, 100.0) == capi.DEKF_ERR_INVALID
    assert lib.dekf_get_innovation_gate(None, None, None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID


def test_c99_client_calls_both_symbols(tmp_path):
    import torch
    body = ("    dekf_params p;\n    dekf_handle h = 0;\n    double g = -1.0;\n    dekf_default_params(&p);\n"
            "    int st = dekf_create(&p, 4, 0, 0, &h);\n"
            '    printf("create %d set %d get %d\\n", st, dekf_set_innovation_gate(h, 16.27), dekf_get_innovation_gate(h, &g, 0, DEKF_HOST));\n'
            '    printf("gate %g\\n", g);\n'
            "    if (st == 0) dekf_destroy(h);\n")
    if torch.cuda.is_available():   # (an ADMM handle: the gate is refused, the bound reads 0)
        expect = f"create 0 set {capi.DEKF_ERR_INVALID} get {capi.DEKF_OK}\ngate 0"
    else:                           # no device, no handle: dekf_create still answers DEKF_ERR_NO_DEVICE
        expect = f"create {capi.DEKF_ERR_NO_DEVICE} set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID}\ngate -1"
    DL.check_c99_client(tmp_path, "gate_client", body, expect)


# ------------------------------------------------------------------ resource remarks
GATE_USAGE = os.path.join(DL.CSRC, "libdekf_gate_resource_usage.txt")


def test_the_eight_gate_kernels_are_at_their_design_point():
    """libdekf_gate_resource_usage.txt holds the eight gate kernels and nothing else: no spills, no scratch, at most 72 VGPRs (the
    direct kernels' class), no static LDS"""
    import re
    from test_resource_usage import _sources_mtime, parse_usage
    assert os.path.exists(GATE_USAGE) and os.path.getmtime(GATE_USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(GATE_USAGE).read()
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    table = parse_usage(text)
    assert sorted(table) == sorted(GL.GATE_KERNELS)
    for n in GL.GATE_KERNELS:
        u = table[n]
        print(n, u)
        assert u["spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0 and u["vgprs"] + (u["agprs"] or 0) <= IL.MAX_VGPRS, (n, u)
        assert static_lds[n] == 0, n
