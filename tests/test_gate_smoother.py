"""The window of a gating handle (dekf_set_gate_smoother, mhe_gate_window_core.h) without a GPU: the lane-sequential build of the core
against the reference of gate_smooth_lib at two gates per case, the bit contracts (against the gate harness without the option and
against a smoothing innovation run without the gate on the edited log), a stand-alone sanitizer program, the C boundary and the
compiler's account of the eight kernels."""
import os
import re

import numpy as np
import pytest

import direct_lib as DL
import gate_lib as GL
import gate_smooth_lib as GS
import innov_lib as IL
from decentralized_ekf_mhe_amd import capi

NAMES = list(GL.CASES)


# ------------------------------------------------------------------ the reference
def test_low_gate_reference_gates_at_tick_one():
    """at the low gate the reference gates at tick 1 in all four cases (K = 2: a single backward step), and the gated pairs of a case
    are those gate_lib's reference gates"""
    first = {"go1": (1, 1, 1), "cassie": (1, 1, 1), "pogox": (1, 1, 0)}
    for name in NAMES:
        p, s, gate, ref = GS.case_reference(name, "low")
        GL.check_margin(ref, gate, name)
        dec = GL.decisions(ref)
        assert dec == GL.decisions(GL.case_reference(name, "low")[3]), name
        print(name, len(dec), "gated pairs, the first", dec[0])
        assert dec[0][0] == 1, (name, dec[0])
        if name in first:
            assert first[name] in dec, (name, dec[:4])
        else:  # the tripod: two legs of both robots
            assert all(sum(1 for d in dec if d[:2] == (1, b)) == 2 for b in ref), dec[:6]
    assert [len(GL.decisions(GS.case_reference(n, "low")[3])) for n in ("go1", "cassie", "tripod", "pogox")] == [19, 31, 57, 13]


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_core_against_the_reference(name, which):
    """every tick of every instance: the decisions and the newest block as gate_lib holds them, and every window block within the direct
    solve's yardsticks (XREL / XABS per 3-block, CREL) of the optimum of the window QP with the gated legs' swing blocks and the
    diagonal blocks of its KKT inverse.  The worst errors of the gated and the ungated ticks are printed"""
    p, s, gate, ref = GS.case_reference(name, which)
    GL.check_margin(ref, gate, name)
    run = GS.case_sim(name, which)
    GL.check_against_reference(run, ref, list(ref), (name, which))
    worst = GS.check_window_against_reference(run, ref, list(ref), (name, which))
    print(name, which, {kind: f"x {v[0]:.2e} of the yardstick, cov {v[1]:.2e}" for kind, v in sorted(worst.items())})
    assert "gated" in worst and "ungated" in worst


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("name", NAMES)
def test_a_gate_that_never_fires_is_a_smoothing_innovation_handle(name):
    never, off = GS.case_sim(name, "never"), GS.case_sim(name, "off")
    assert len(never) == len(off)
    for a, b in zip(never, off):
        assert not a["gated"].any()
        assert a["K"] == b["K"]
        for key in GL.OUTPUTS + ("qm",) + GS.WINDOW:
            assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_everything_but_the_window_is_the_gate_without_the_option(name, which):
    """x_mhe, v_b, status, Cov(x_T), the five arrays, gated and the newest record's Q_m words: the bits of the gate harness"""
    with_option, without = GS.case_sim(name, which), GL.case_sim(name, which)
    assert len(with_option) == len(without)
    for k, (a, b) in enumerate(zip(with_option, without)):
        for key in GL.OUTPUTS + ("gated", "qm"):
            assert np.array_equal(a[key], b[key], equal_nan=True), (name, k + 1, key)


@pytest.mark.parametrize("which", ["high", "low"])
@pytest.mark.parametrize("name", NAMES)
def test_window_bits(name, which):
    """at every tick at which an instance gates nothing, every output, x_win and cov_win included, is the bits of a smoothing innovation
    run without the gate fed the log with contact = 0 at the pairs gated before; at a gated tick x_win[K-1] is x_mhe and cov_win[K-1]
    the covariance block to the bit, every cov_win[k] is symmetric to the bit; entries k >= K keep FILL at every tick"""
    p, B, K, sub, s = GL.case_streams(name)
    _, _, gate, ref = GS.case_reference(name, which)
    run = GS.case_sim(name, which)
    dec = GL.decisions(ref)
    behind = GL.check_bits_on_ungated_ticks(run, lambda so, n: GS.run_sim(p, so, n, K), s, dec, B, K, (name, which),
                                            GL.OUTPUTS + GS.WINDOW)
    assert behind > 0
    assert GS.check_window_bits_at_gated_ticks(run, (name, which)) == len({d[:2] for d in dec})
    for g in run:
        assert (g["xw"][:, g["K"]:] == DL.FILL).all() and (g["cw"][:, g["K"]:] == DL.FILL).all()
        assert np.isfinite(g["xw"][:, :g["K"]]).all() and np.isfinite(g["cw"][:, :g["K"]]).all()


def test_the_correction_widens_every_covariance():
    """C is positive definite, so P_k' - P_k is positive semi-definite at every window step of a gated tick: the corrected window against
    the window of the smoothing run that has not seen this tick's edit (the same records up to this tick)"""
    name, which = "go1", "low"
    p, B, K, sub, s = GL.case_streams(name)
    run = GS.case_sim(name, which)
    dec = GL.decisions(GS.case_reference(name, which)[3])
    seen = 0
    for b in range(B):
        ticks, so = GL.edited_copies(s, b, B, dec)
        off = GS.run_sim(p, so, len(ticks) + 1, K)
        for i, k in enumerate(ticks):
            g, o = run[k - 1], off[k - 1]
            for j in range(g["K"]):
                d = g["cw"][b][j] - o["cw"][i][j]
                scale = np.sqrt(np.abs(np.diag(o["cw"][i][j])))
                assert np.linalg.eigvalsh(d / scale[:, None] / scale[None, :]).min() >= -1e-9, (b, k, j)
                seen += 1
    assert seen > 0


def test_a_failed_solve_gates_nothing_and_keeps_the_smoothers_nan_window():
    """an instance whose solve failed (a poisoned sample) gates nothing: its window is the smoothing kernel's, NaN in all K entries;
    its neighbour keeps its bits, window included"""
    p, B, K, sub, s = GL.case_streams("go1")
    gate = GL.CASES["go1"][2]
    clean = GS.run_sim(p, s, B, 30, gate)
    sp = GL.copy_streams(s)
    sp["accel"][24, 0, 0] = np.nan
    pois = GS.run_sim(p, sp, B, 30, gate)
    g = pois[23]
    assert g["status"][0] == capi.DEKF_SOLVE_NUMERIC and not g["gated"][0].any()
    assert np.isnan(g["xw"][0][:g["K"]]).all() and np.isnan(g["cw"][0][:g["K"]]).all()
    for a, b in zip(clean, pois):
        for key in ("gated", "x", "xw", "cw"):
            assert np.array_equal(a[key][1], b[key][1]), key


def test_a_failed_correction_gives_nan_in_all_k_entries():
    """the core behind a correction that failed (the gate's DEKF_SOLVE_NUMERIC path, which no valid input of the harness reaches, so
    the core is called with that flag): NaN in the K first entries of both arrays of the instance, every other entry untouched"""
    p, B, K, sub, s = GL.case_streams("go1")
    sim = GS.GateSmoothSim(p, B, GL.CASES["go1"][2])
    ns, N = p.dim_state, p.N
    for Kw in (2, 7, N):
        xw, cw = np.full((B, N, ns), DL.FILL), np.full((B, N, ns, ns), DL.FILL)
        sim.L.hs_gate_window_failed(sim.h, 1, Kw, GS.HL._p(xw), GS.HL._p(cw))
        assert np.isnan(xw[1, :Kw]).all() and np.isnan(cw[1, :Kw]).all()
        assert (xw[1, Kw:] == DL.FILL).all() and (cw[1, Kw:] == DL.FILL).all() and (xw[0] == DL.FILL).all() and (cw[0] == DL.FILL).all()


# ------------------------------------------------------------------ sanitizers
ASAN_BUFFERS = """    const int nm = 3 * L;
    std::vector<double> nu((size_t)B * nm, -7.0), S((size_t)B * nm * nm, -7.0), nis(B, -7.0), nl((size_t)B * L, -7.0), ll(B, -7.0);
    std::vector<double> xw((size_t)B * N * ns, -7.0), cw((size_t)B * N * ns * ns, -7.0);
    std::vector<int> gated((size_t)B * L, -7);
    int fired = 0;
"""
ASAN_UPDATE = """        // every seventh step a gate that every stance leg passes, else one that a leg passes now and then
        if (hs_update_direct_smooth_innov_gate(h, T, T % 7 == 3 ? 1e-3 : 40.0, cov.data(), xw.data(), cw.data(), nu.data(), S.data(), nis.data(),
                                               nl.data(), ll.data(), gated.data())) return 3;
        const int Kw = T + 1 < N ? T + 1 : N;
        for (int b = 0; b < B; ++b) {
            int any = 0;
            for (int i = 0; i < L; ++i) any += gated[(size_t)b * L + i];
            fired += any;
            // (the backward pass mirrors its blocks and the gate its newest one: symmetric to the bit; the newest block is Cov(x_T))
            for (int k = 0; k < Kw; ++k)
                for (int i = 0; i < ns; ++i)
                    for (int j = 0; j < ns; ++j) {
                        const double v = cw[(((size_t)b * N + k) * ns + i) * ns + j];
                        if (any || k < Kw - 1) bad += !(v == cw[(((size_t)b * N + k) * ns + j) * ns + i]);
                        if (k == Kw - 1) bad += !(v == cov[((size_t)b * ns + i) * ns + j]);
                    }
        }
"""
ASAN_REPORT = """    std::printf("%d legs gated, %d bad entries\\n", fired, bad);
    if (!fired) return 4;
"""


def test_window_core_clean_under_asan_ubsan(tmp_path, monkeypatch):
    """a stand-alone program over gate_smooth_hostsim.cpp under AddressSanitizer + UBSan (CPU build, run directly): the window correction
    on gated ticks of Go1 (L = 4), a two-leg robot and the one-leg case, through the window fill, full windows and VO rows"""
    driver = DL.ASAN_DRIVER.replace('#include "direct_hostsim.cpp"', '#include "gate_smooth_hostsim.cpp"')
    main = "int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }"
    assert main in driver
    driver = driver.replace(main, "int main() { return run(4, 3, 20, 50, 0, 0) | run(2, 5, 6, 24, 0, 0) | run(1, 2, 30, 44, 0, 0); }")
    monkeypatch.setattr(DL, "ASAN_DRIVER", driver)
    DL.check_clean_under_asan_ubsan(tmp_path, "gate_smooth_driver", ASAN_BUFFERS, ASAN_UPDATE, ASAN_REPORT)


# ------------------------------------------------------------------ the C boundary
SYMBOLS = ("dekf_set_gate_smoother",)


def test_header_declares_the_call_and_states_the_scope():
    hdr = DL.header()
    assert "dekf_status dekf_set_gate_smoother(dekf_handle h, int on);" in hdr
    text = hdr[hdr.index("the window of a gating handle (opt-in"):]
    text = text[:text.index("dekf_status dekf_set_gate_smoother")]
    for phrase in ("x_win[b][K-1] is\n * bit-identical to x_mhe[b]", "symmetric to the\n * bit", "dekf_set_window_cross(h, 1) is DEKF_ERR_INVALID",
                   "Not part of this interface: cross-covariances of a gating handle; ADMM and KF handles; leg_odom_type 1"):
        assert phrase in text, phrase
    # the gate's section keeps its sentences
    gate = hdr[hdr.index("innovation gate (opt-in"):hdr.index("the window of a gating handle (opt-in")]
    assert "the window of a gating handle is\n * not part of this interface" in gate


def test_library_exports_and_binding_lists_it():
    DL.check_exports_and_binding(SYMBOLS)


def test_abi_version_and_params_layout_unchanged():
    DL.check_abi_version_and_params_layout()


def test_null_handle_is_invalid():
    lib = capi.load()
    assert lib.dekf_set_gate_smoother(None, 1) == capi.DEKF_ERR_INVALID
    assert lib.dekf_set_gate_smoother(None, 0) == capi.DEKF_ERR_INVALID


def test_c99_client_calls_the_symbol(tmp_path):
    import torch
    body = ("    dekf_params p;\n    dekf_handle h = 0;\n    dekf_default_params(&p);\n"
            "    int st = dekf_create(&p, 4, 0, 0, &h);\n"
            '    printf("create %d on %d off %d\\n", st, dekf_set_gate_smoother(h, 1), dekf_set_gate_smoother(h, 0));\n'
            "    if (st == 0) dekf_destroy(h);\n")
    if torch.cuda.is_available():   # (an ADMM handle: no gate, so the option is refused; switching it off is a no-op)
        expect = f"create 0 on {capi.DEKF_ERR_INVALID} off {capi.DEKF_OK}"
    else:                           # no device, no handle
        expect = f"create {capi.DEKF_ERR_NO_DEVICE} on {capi.DEKF_ERR_INVALID} off {capi.DEKF_ERR_INVALID}"
    DL.check_c99_client(tmp_path, "gate_smoother_client", body, expect)


# ------------------------------------------------------------------ resource remarks
USAGE = os.path.join(DL.CSRC, "libdekf_gate_smooth_resource_usage.txt")


def test_the_eight_kernels_are_at_their_design_point():
    """libdekf_gate_smooth_resource_usage.txt holds the eight new kernels and nothing else: no spills, no scratch, at most 72 VGPRs (the
    direct kernels' class), no static LDS"""
    from test_resource_usage import _sources_mtime, parse_usage
    assert os.path.exists(USAGE) and os.path.getmtime(USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(USAGE).read()
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    table = parse_usage(text)
    assert sorted(table) == sorted(GS.KERNELS)
    for n in GS.KERNELS:
        u = table[n]
        print(n, u)
        assert u["spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0 and u["vgprs"] + (u["agprs"] or 0) <= IL.MAX_VGPRS, (n, u)
        assert static_lds[n] == 0, n
