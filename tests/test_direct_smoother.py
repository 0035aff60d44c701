"""The window smoother of the direct MHE solve (dekf_set_smoother / dekf_get_window, csrc/mhe_direct_core.h: SMOOTH) without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the C++ shim compiles with robot_params::smoothWindow_; the ten smoothing twins sit at their design point.
Core: the lane-sequential build of the SMOOTH instantiation (tests/hostsim/direct_smooth_hostsim.cpp) on the records and the input
snapshot that the assemble step leaves: EVERY block of the window, every checked tick, against the exact optimum of the oracle's QP
(ref_numpy.kkt_exact) and the diagonal blocks of the inverse of that QP's KKT matrix, inside test_direct_solve.py's yardstick; the newest
block bit-equal to what the non-smoothing core returns; without VO rows against the same references."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hostsim_lib as HL
import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params
from decentralized_ekf_mhe_amd.params import DekfParams
from decentralized_ekf_mhe_amd.streams import make_streams
from test_direct_solve import (CORE_CASES, CREL, CSRC, HOSTSIM, ROOT, XABS, XREL, _params, block_err, blocks3, cov_err, rough_streams,
                               run_direct_sim, vo_equalities)

SYMBOLS = ("dekf_set_smoother", "dekf_get_window")
KERNELS = [f"k_mhe_solve_direct_{s}" for s in ("4_n20", "2_n20", "1", "2", "3", "4", "foot_1", "foot_2", "foot_3", "foot_4")]


def window_reference(p, s, b, ticks, arrival=None):
    """{tick: (x [K][ns], Cov [K][ns][ns], VO equality rows)} of instance b: the state blocks of the exact optimum of the oracle's
    window QP (kkt_exact) and the diagonal state blocks of the (1, 1) block of the inverse of its KKT matrix, equilibrated as
    kkt_exact does (test_direct_solve.exact_reference for every block), read at the state offsets of SURVEY.md Appendix A.
    arrival: {tick: (M_p, n_p)} put in place of the oracle's arrival cost on the first block"""
    ns, nm = p.dim_state, 3 * p.num_legs
    sv = 2 * ns + nm + 3
    pipe = O.Pipe(p)
    out = {}
    for k in range(max(ticks) + 1):
        pipe.feed(s, k, b)
        pipe.step(k)
        if k not in ticks:
            continue
        H, g, A, l, u = pipe.est.qp()
        if arrival is not None:
            H, g = H.copy(), g.copy()
            H[:ns, :ns], g[:ns] = arrival[k]
        n = H.shape[0]
        K = (n - ns - nm) // sv + 1
        assert K == min(k + 1, p.N) and (ns + nm) + (K - 1) * sv == n

        def xo(j):
            return 0 if j == 0 else (ns + nm) + (j - 1) * sv + ns + 3

        assert xo(K - 1) == n - ns - nm   # (the slice test_direct_solve.exact_reference reads)
        x, _ = RN.kkt_exact(H, g, A, l, u)
        eq = (u - l) < 1e-9
        Ae = A[eq]
        KK = np.zeros((n + Ae.shape[0],) * 2)
        KK[:n, :n], KK[:n, n:], KK[n:, :n] = H, Ae.T, Ae
        d = 1.0 / np.sqrt(np.maximum(np.abs(KK).max(axis=1), 1e-300))
        Ki = np.linalg.inv(KK * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
        X = np.array([x[xo(j):xo(j) + ns] for j in range(K)])
        Cv = np.array([Ki[xo(j):xo(j) + ns, xo(j):xo(j) + ns] for j in range(K)])
        out[k] = (X, Cv, vo_equalities(p, A, l))
    return out


def window_errors(xw, cw, X, Cv, ns):
    """worst x error (units of the yardstick) and covariance error over the blocks of one window, and the block of the worst x error"""
    ex = [block_err(xw[j], X[j], blocks3(ns), XREL, XABS) for j in range(len(X))]
    ec = [cov_err(cw[j], Cv[j]) for j in range(len(X))]
    return max(ex), max(ec), int(np.argmax(ex))


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = open(os.path.join(ROOT, "include", "dekf.h")).read()
    assert re.search(r"dekf_status\s+dekf_set_smoother\s*\(\s*dekf_handle\s+h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_window\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*steps\s*,\s*double\s*\*\s*x_win\s*,\s*double\s*\*\s*"
                     r"cov_win\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)


def test_library_exports_and_binding_lists_them():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    assert capi.PROTOTYPES["dekf_set_smoother"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_window"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    lib = capi.load()
    assert lib.dekf_abi_version() == capi.DEKF_ABI_VERSION == 4
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    assert bytes(p) == bytes(go1_params())


def test_null_handle_is_invalid():
    lib = capi.load()
    for on in (0, 1, 2):
        assert lib.dekf_set_smoother(None, on) == capi.DEKF_ERR_INVALID
    k = C.c_int(-7)
    x = (C.c_double * 9)()
    assert lib.dekf_get_window(None, C.cast(C.byref(k), C.c_void_p), C.cast(x, C.c_void_p), None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    assert k.value == -7


def test_header_compiles_as_c99_with_the_smoother_calls(tmp_path):
    src = tmp_path / "smoother_client.c"
    src.write_text(
        '#include <stdio.h>\n#include "dekf.h"\n'
        "int main(void) {\n"
        "    double x[9], cov[81];\n"
        "    int steps = 0;\n"
        "    dekf_status a = dekf_set_smoother((dekf_handle)0, 1);\n"
        "    dekf_status b = dekf_get_window((dekf_handle)0, &steps, x, cov, DEKF_HOST);\n"
        '    printf("set %d get %d steps %d abi %d\\n", (int)a, (int)b, steps, DEKF_ABI_VERSION);\n'
        "    return 0;\n}\n")
    exe = tmp_path / "smoother_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-ldekf", f"-Wl,-rpath,{CSRC}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} steps 0 abi 4" in out.stdout, out.stdout


def shim_smooth_source():
    """examples/go1_shim_demo.cpp with robot_params::directSolve_ and smoothWindow_ set; behind every line's 9 + 3 + ... columns it prints
    window_steps_, then x_window_ and C_window_ of every window step"""
    src = open(os.path.join(ROOT, "examples", "go1_shim_demo.cpp")).read()
    src = src.replace('#include "../decentralized_ekf_mhe_amd/cpp/DecentralEst.hpp"',
                      '#include "' + os.path.join(ROOT, "decentralized_ekf_mhe_amd", "cpp", "DecentralEst.hpp") + '"')
    anchor = "    if (argc > 3) params->est_type_ = std::atoi(argv[3]);\n"
    assert anchor in src
    src = src.replace(anchor, anchor + "    params->directSolve_ = true;\n    params->smoothWindow_ = true;\n")
    anchor = '        std::printf(" %d\\n", mhe.solver_iters_);\n'
    assert anchor in src
    src = src.replace(anchor,
                      "        for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_MHE_(i / 9, i % 9));\n"
                      "        std::printf(\" %d\", mhe.window_steps_);\n"
                      "        for (int k = 0; k < mhe.window_steps_; ++k) {\n"
                      "            for (int i = 0; i < 9; ++i) std::printf(\" %.17g\", mhe.x_window_[(size_t)k](i));\n"
                      "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_window_[(size_t)k](i / 9, i % 9));\n"
                      "        }\n" + anchor)
    return src


def build_shim_smooth(tmp_path):
    src = tmp_path / "shim_smooth.cpp"
    src.write_text(shim_smooth_source())
    exe = str(tmp_path / "shim_smooth")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", str(src), "-o", exe, "-L" + CSRC, "-ldekf",
                           "-Wl,-rpath," + CSRC, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_compiles_with_smooth_window(tmp_path):
    exe = build_shim_smooth(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_smoothing_twins_at_their_design_point():
    """every direct kernel has its _smooth twin in the product build; no spills, no scratch, no static LDS (the
    dynamic LDS is DirectScratch::len for both, so the twins keep the LDS residency of section 4.8); and the twin's occupancy class
    (wavefronts per SIMD as far as registers go) is not below its non-smoothing twin's — or, where it is (k_mhe_solve_direct_foot_1_smooth:
    7 against 8, over the scalar registers), it is still above what the kernel's LDS admits, which then decides the residency of both"""
    from test_resource_usage import USAGE, _sources_mtime, parse_usage
    assert os.path.exists(USAGE) and os.path.getmtime(USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(USAGE).read()
    table = parse_usage(text)
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    for n, (L, ft) in zip(KERNELS, [(4, 0), (2, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (3, 1), (4, 1)]):
        assert n in table and n + "_smooth" in table, n
        u, t = table[n], table[n + "_smooth"]
        print(n + "_smooth", t)
        assert t["spill"] == 0 and t["scratch"] == 0 and static_lds[n + "_smooth"] == 0, (n, t)
        ns = 9 + 3 * L * ft
        granule = 1536
        lds_per_simd = (160 * 1024) // (((5 * ns * ns + 6 * ns + 8) * 8 + granule - 1) // granule * granule) / 4.0
        assert t["occupancy"] >= u["occupancy"] or t["occupancy"] >= lds_per_simd, (n, t, u, lds_per_simd)


# ------------------------------------------------------------------ 2: the core, lane-sequential
LIB = os.path.join(HOSTSIM, "libdirect_smooth_hostsim.so")


def build_smooth_hostsim():
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "direct_smooth_hostsim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                               os.path.join(HOSTSIM, "direct_smooth_hostsim.cpp")])
    return LIB


_libs = {}


def smooth_lib():
    if "lib" not in _libs:
        L = HL._bind(C.CDLL(build_smooth_hostsim()))
        L.hs_update_direct_smooth.argtypes = [C.c_void_p, C.c_int, HL._dp, HL._dp, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


FILL = -12345.0   # what the window buffers hold before an update: entries k >= K must keep it


class SmoothSim(HL.HostSim):
    """hostsim_lib.HostSim on the smoothing harness: step(T) runs the assemble step and the SMOOTH core, and keeps Cov(x_T), K and the
    window arrays ([B][N][...], pre-filled with FILL)"""

    def __init__(self, params, batch):
        self.p, self.B, self.L = params, batch, smooth_lib()
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.cov = self.xw = self.cw = None
        self.K = 0

    def step(self, T):
        self.L.hs_ekf_step(self.h)
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        ns, N = self.p.dim_state, self.p.N
        self.cov = np.zeros((self.B, ns, ns))
        self.xw, self.cw = np.full((self.B, N, ns), FILL), np.full((self.B, N, ns, ns), FILL)
        self.L.hs_update_direct_smooth(self.h, T, HL._p(self.cov), HL._p(self.xw), HL._p(self.cw))
        self.K = min(T + 1, N)


def run_smooth_sim(p, s, B, K, ticks):
    sim = SmoothSim(p, B)
    out = {}
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k in ticks:
            M, n = sim.arrival()
            out[k] = dict(sim.get(), cov=sim.cov.copy(), M=M, n=n, K=sim.K, xw=sim.xw.copy(), cw=sim.cw.copy())
    return out


@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_every_window_block_is_the_exact_optimum_of_the_oracle_qp(name):
    mk, B, K, ticks = CORE_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    got = run_smooth_sim(p, s, B, K, set(ticks))
    plain = run_direct_sim(p, s, B, K, set(ticks))
    ns, N = p.dim_state, p.N
    own_arrival = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    worst_x, worst_c, worst_blk, vo_eq = 0.0, 0.0, None, 0
    for b in range(B):
        arrival = {k: (got[k]["M"][b], got[k]["n"][b]) for k in ticks if k >= N} if own_arrival else None
        ref = window_reference(p, s, b, set(ticks))
        ref_own = window_reference(p, s, b, {k for k in ticks if k >= N}, arrival=arrival) if arrival else {}
        for k in ticks:
            X, Cv, nv = ref_own.get(k, ref[k])
            g, Kw = got[k], got[k]["K"]
            assert Kw == min(k + 1, N) == len(X)
            assert g["status"][b] == capi.DEKF_SOLVE_OK
            # everything the non-smoothing core writes: the same bits; the newest block of the window: those bits again
            for key in ("x", "v_b", "status", "iters", "cov"):
                assert np.array_equal(g[key], plain[k][key]), (k, key)
            assert np.array_equal(g["xw"][b, Kw - 1], plain[k]["x"][b]), k
            assert np.array_equal(g["cw"][b, Kw - 1], plain[k]["cov"][b]), k
            assert (g["xw"][b, Kw:] == FILL).all() and (g["cw"][b, Kw:] == FILL).all(), k
            cw = g["cw"][b, :Kw]
            assert np.array_equal(cw[:Kw - 1], np.swapaxes(cw[:Kw - 1], -1, -2)), k   # symmetric, both triangles
            ex, ec, blk = window_errors(g["xw"][b, :Kw], cw, X, Cv, ns)
            if ex > worst_x:
                worst_blk = (k, blk, Kw)
            worst_x, worst_c, vo_eq = max(worst_x, ex), max(worst_c, ec), vo_eq + nv
    print(f"[{name}] every window block: worst x error {worst_x:.3g} x (1e-8 rel + 1e-10) at (tick, block, K) = {worst_blk}; worst "
          f"covariance error {worst_c:.3g} sqrt(C_ii C_jj); VO equality rows in the checked windows: {vo_eq}")
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert worst_x <= 1.0
    assert worst_c <= CREL


@pytest.mark.parametrize("name,maker", [("go1", lambda: _params(go1_params)), ("cassie", lambda: _params(cassie_params))])
def test_core_without_vo_every_window_block(name, maker):
    """no VO row (make_streams(vo=False)): the fixed-interval Kalman smoother on the window; every block against the same references"""
    p = maker()
    B, K = 2, 2 * p.N + 5
    ticks = [3, p.N - 1, p.N, p.N + 7, K - 1]
    s = make_streams(p, B, K, vo=False)
    got = run_smooth_sim(p, s, B, K, set(ticks))
    worst_x, worst_c = 0.0, 0.0
    for b in range(B):
        ref = window_reference(p, s, b, set(ticks))
        for k in ticks:
            X, Cv, nv = ref[k]
            assert nv == 0
            Kw = got[k]["K"]
            ex, ec, _ = window_errors(got[k]["xw"][b, :Kw], got[k]["cw"][b, :Kw], X, Cv, p.dim_state)
            worst_x, worst_c = max(worst_x, ex), max(worst_c, ec)
    print(f"[{name}, no VO] every window block: worst x error {worst_x:.3g} x, worst covariance error {worst_c:.3g}")
    assert worst_x <= 1.0
    assert worst_c <= CREL


ASAN_DRIVER = r"""
#include "direct_smooth_hostsim.cpp"
#include <cmath>
#include <cstdio>
// synthetic sensors as in test_direct_solve.py's driver, VO on every sixth step: window fill, marginalisation and VO rows.  The window
// buffers are allocated at exactly [B][N][...] and the guard behind the K written entries is checked, so that an index past the
// window is caught by the sanitizer or by the guard.
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 2;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns);
    std::vector<int> mask(B, 1); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    int bad = 0;
    std::vector<double> xw, cw;
    for (int T = 0; T < steps; ++T) {
        for (int b = 0; b < B; ++b) {
            t[b] = 0.005 * T + 1e-5 * b;
            acc[3*b] = 0.1; acc[3*b+1] = -0.05; acc[3*b+2] = 9.8; gy[3*b] = 0.01; gy[3*b+1] = 0.02; gy[3*b+2] = 0.2;
            for (int i = 0; i < 3 * L; ++i) pf[3*L*b + i] = 0.1 * (i % 3) - 0.25;
            for (int i = 0; i < 3 * L * nj; ++i) J[3*L*nj*b + i] = (i % (nj + 1) == 0) ? 0.2 : 0.03 * ((i + T) % 5);
            for (int i = 0; i < L * nj; ++i) qd[L*nj*b + i] = 0.1 * ((i + T) % 7) - 0.3;
            for (int i = 0; i < L; ++i) c[L*b + i] = ((T / 5 + i) % 2) ? 1.0 : 0.0;
            tp[b] = 0.005 * (T - 7); tn[b] = 0.005 * (T - 1); dp[3*b] = 0.003; dp[3*b+1] = 0; dp[3*b+2] = 0;
            q[4*b] = 1; q[4*b+1] = q[4*b+2] = q[4*b+3] = 0;
        }
        hs_push_imu(h, t.data(), acc.data(), gy.data());
        hs_push_leg(h, pf.data(), J.data(), qd.data(), c.data());
        if (T > 8 && T % 6 == 0) hs_push_vo(h, mask.data(), tp.data(), tn.data(), dp.data(), tn.data(), q.data());
        hs_ekf_step(h);
        if (T == 0) { hs_initialize(h); continue; }
        xw.assign((size_t)B * N * ns, -7.0);
        cw.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_smooth(h, T, cov.data(), xw.data(), cw.data());
        const int K = T + 1 < N ? T + 1 : N;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < N; ++k) {
                for (int i = 0; i < ns; ++i) { const double v = xw[((size_t)b * N + k) * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int i = 0; i < ns * ns; ++i) { const double v = cw[((size_t)b * N + k) * ns * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
            }
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d v=%g oldest v=%g cov00=%g, %d bad window entries\n", L, nj, N, ft,
                form, st[0], x[3], xw[3], cw[0], bad);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && bad == 0 ? 0 : 2;
}
int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }
"""


def test_smooth_core_clean_under_asan_ubsan(tmp_path):
    """the SMOOTH core under AddressSanitizer + UBSan (CPU build): Go1 and foot states (both arrival-cost forms) through window fill,
    marginalisation and VO rows, the window buffers exactly as large as the contract says"""
    src = tmp_path / "smooth_driver.cpp"
    src.write_text(ASAN_DRIVER)
    exe = tmp_path / "smooth_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
