"""The window cross-covariances of the direct smoother (dekf_set_window_cross / dekf_get_window_cross, csrc/mhe_direct_core.h: CROSS)
without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the C++ shim compiles with robot_params::windowCross_; the ten _smooth_cross twins sit at their design point.
Core: the lane-sequential build of the CROSS instantiation (tests/hostsim/direct_cross_hostsim.cpp) on the records and the input
snapshot that the assemble step leaves: EVERY written block of cov_lag1 and cov_newest, every checked tick, against the matching
off-diagonal block of the inverse of the oracle QP's KKT matrix (test_direct_smoother.window_reference's construction, for every pair
of window states), in units of sqrt(Cov(x_a)_ii Cov(x_b)_jj) and inside CREL; the two bit identities of the new arrays; everything
the SMOOTH core writes unchanged to the bit; without VO rows the Kalman smoother's cross-covariances."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hostsim_lib as HL
import oracle_lib as O
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params
from decentralized_ekf_mhe_amd.estimator import relative_cov
from decentralized_ekf_mhe_amd.params import DekfParams
from decentralized_ekf_mhe_amd.streams import make_streams
from test_direct_smoother import FILL, KERNELS, run_smooth_sim
from test_direct_solve import CORE_CASES, CREL, CSRC, HOSTSIM, ROOT, _params, rough_streams, vo_equalities

SYMBOLS = ("dekf_set_window_cross", "dekf_get_window_cross")


def cross_reference(p, s, b, ticks, arrival=None):
    """{tick: (Cov [K][K][ns][ns], VO equality rows)} of instance b: EVERY state block pair (a, c) -> Cov(x_a, x_c) of the (1, 1) block
    of the inverse of the oracle window QP's KKT matrix, equilibrated as kkt_exact does (test_direct_smoother.window_reference extended
    to all index pairs), read at the state offsets of SURVEY.md Appendix A.
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
            H = H.copy()
            H[:ns, :ns] = arrival[k][0]
        n = H.shape[0]
        K = (n - ns - nm) // sv + 1
        assert K == min(k + 1, p.N) and (ns + nm) + (K - 1) * sv == n
        xo = [0 if j == 0 else (ns + nm) + (j - 1) * sv + ns + 3 for j in range(K)]
        assert xo[K - 1] == n - ns - nm
        eq = (u - l) < 1e-9
        Ae = A[eq]
        KK = np.zeros((n + Ae.shape[0],) * 2)
        KK[:n, :n], KK[:n, n:], KK[n:, :n] = H, Ae.T, Ae
        d = 1.0 / np.sqrt(np.maximum(np.abs(KK).max(axis=1), 1e-300))
        Ki = np.linalg.inv(KK * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
        idx = np.concatenate([np.arange(o, o + ns) for o in xo])
        Cf = Ki[np.ix_(idx, idx)].reshape(K, ns, K, ns).transpose(0, 2, 1, 3).copy()
        out[k] = (Cf, vo_equalities(p, A, l))
    return out


def pair_err(got, Cf, a, c):
    """|got - Cov(x_a, x_c)|_ij / sqrt(Cov(x_a)_ii Cov(x_c)_jj), worst entry, the scales from the reference's diagonal blocks"""
    da, dc = np.sqrt(np.abs(np.diagonal(Cf[a, a]))), np.sqrt(np.abs(np.diagonal(Cf[c, c])))
    return float((np.abs(got - Cf[a, c]) / (da[:, None] * dc[None, :])).max())


def cross_errors(l1, zn, Cf):
    """worst error of the K - 1 lag-one and the K to-newest blocks of one window"""
    K = Cf.shape[0]
    e1 = max(pair_err(l1[k], Cf, k, k + 1) for k in range(K - 1))
    en = max(pair_err(zn[k], Cf, k, K - 1) for k in range(K))
    return e1, en


# ------------------------------------------------------------------ 1: the C boundary
def test_header_declares_both_calls():
    hdr = open(os.path.join(ROOT, "include", "dekf.h")).read()
    assert re.search(r"dekf_status\s+dekf_set_window_cross\s*\(\s*dekf_handle\s+h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_window_cross\s*\(\s*dekf_handle\s+h\s*,\s*int\s*\*\s*steps\s*,\s*double\s*\*\s*cov_lag1\s*,\s*"
                     r"double\s*\*\s*cov_newest\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_ABI_VERSION\s+4\b", hdr)
    assert "Not part of this interface: the lag-one" not in hdr


def test_library_exports_and_binding_lists_them():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    assert capi.PROTOTYPES["dekf_set_window_cross"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_window_cross"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    lib = capi.load()
    assert lib.dekf_abi_version() == capi.DEKF_ABI_VERSION == 4
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    assert bytes(p) == bytes(go1_params())


def test_null_handle_is_invalid():
    lib = capi.load()
    for on in (0, 1, 2):
        assert lib.dekf_set_window_cross(None, on) == capi.DEKF_ERR_INVALID
    k = C.c_int(-7)
    x = (C.c_double * 81)()
    assert lib.dekf_get_window_cross(None, C.cast(C.byref(k), C.c_void_p), C.cast(x, C.c_void_p), None, capi.DEKF_HOST) == capi.DEKF_ERR_INVALID
    assert k.value == -7


def test_header_compiles_as_c99_with_the_cross_calls(tmp_path):
    src = tmp_path / "cross_client.c"
    src.write_text(
        '#include <stdio.h>\n#include "dekf.h"\n'
        "int main(void) {\n"
        "    double lag1[81], newest[81];\n"
        "    int steps = 0;\n"
        "    dekf_status a = dekf_set_window_cross((dekf_handle)0, 1);\n"
        "    dekf_status b = dekf_get_window_cross((dekf_handle)0, &steps, lag1, newest, DEKF_HOST);\n"
        '    printf("set %d get %d steps %d abi %d\\n", (int)a, (int)b, steps, DEKF_ABI_VERSION);\n'
        "    return 0;\n}\n")
    exe = tmp_path / "cross_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-ldekf", f"-Wl,-rpath,{CSRC}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} steps 0 abi 4" in out.stdout, out.stdout


def shim_cross_source():
    """examples/go1_shim_demo.cpp with robot_params::directSolve_, smoothWindow_ and windowCross_ set; behind every line's 9 + 3 + ...
    columns it prints window_steps_, then C_window_, C_newest_ and (but for the newest step) C_lag1_ of every window step"""
    src = open(os.path.join(ROOT, "examples", "go1_shim_demo.cpp")).read()
    src = src.replace('#include "../decentralized_ekf_mhe_amd/cpp/DecentralEst.hpp"',
                      '#include "' + os.path.join(ROOT, "decentralized_ekf_mhe_amd", "cpp", "DecentralEst.hpp") + '"')
    anchor = "    if (argc > 3) params->est_type_ = std::atoi(argv[3]);\n"
    assert anchor in src
    src = src.replace(anchor, anchor + "    params->directSolve_ = true;\n    params->smoothWindow_ = true;\n    params->windowCross_ = true;\n")
    anchor = '        std::printf(" %d\\n", mhe.solver_iters_);\n'
    assert anchor in src
    src = src.replace(anchor,
                      "        std::printf(\" %d\", mhe.window_steps_);\n"
                      "        if (mhe.C_newest_.size() != (size_t)mhe.window_steps_) return 3;\n"
                      "        if (mhe.window_steps_ > 0 && mhe.C_lag1_.size() + 1 != mhe.C_newest_.size()) return 3;\n"
                      "        for (int k = 0; k < mhe.window_steps_; ++k) {\n"
                      "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_window_[(size_t)k](i / 9, i % 9));\n"
                      "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_newest_[(size_t)k](i / 9, i % 9));\n"
                      "            if (k + 1 < mhe.window_steps_)\n"
                      "                for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_lag1_[(size_t)k](i / 9, i % 9));\n"
                      "        }\n" + anchor)
    return src


def build_shim_cross(tmp_path):
    src = tmp_path / "shim_cross.cpp"
    src.write_text(shim_cross_source())
    exe = str(tmp_path / "shim_cross")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", str(src), "-o", exe, "-L" + CSRC, "-ldekf",
                           "-Wl,-rpath," + CSRC, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_compiles_with_window_cross(tmp_path):
    exe = build_shim_cross(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_cross_twins_at_their_design_point():
    """every direct kernel has its _smooth_cross twin in the product build; no spills, no scratch, no static LDS (the dynamic LDS is
    DirectScratch::len for all three, so the twins keep the LDS residency of DESIGN.md section 4.8); and the twin's occupancy class
    (wavefronts per SIMD as far as registers go) is not below its _smooth sibling's, or is still above what the kernel's LDS admits (the
    rule of test_smoothing_twins_at_their_design_point, one twin further)"""
    from test_resource_usage import USAGE, _sources_mtime, parse_usage
    assert os.path.exists(USAGE) and os.path.getmtime(USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(USAGE).read()
    table = parse_usage(text)
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    for n, (L, ft) in zip(KERNELS, [(4, 0), (2, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (3, 1), (4, 1)]):
        assert n + "_smooth" in table and n + "_smooth_cross" in table, n
        u, t = table[n + "_smooth"], table[n + "_smooth_cross"]
        print(n + "_smooth_cross", t)
        assert t["spill"] == 0 and t["scratch"] == 0 and static_lds[n + "_smooth_cross"] == 0, (n, t)
        ns = 9 + 3 * L * ft
        granule = 1536
        lds_per_simd = (160 * 1024) // (((5 * ns * ns + 6 * ns + 8) * 8 + granule - 1) // granule * granule) / 4.0
        assert t["occupancy"] >= u["occupancy"] or t["occupancy"] >= lds_per_simd, (n, t, u, lds_per_simd)


# ------------------------------------------------------------------ 2: the core, lane-sequential
LIB = os.path.join(HOSTSIM, "libdirect_cross_hostsim.so")


def build_cross_hostsim():
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp", "direct_smooth_hostsim.cpp", "direct_cross_hostsim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                               os.path.join(HOSTSIM, "direct_cross_hostsim.cpp")])
    return LIB


_libs = {}


def cross_lib():
    if "lib" not in _libs:
        L = HL._bind(C.CDLL(build_cross_hostsim()))
        L.hs_update_direct_cross.argtypes = [C.c_void_p, C.c_int, HL._dp, HL._dp, HL._dp, HL._dp, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


class CrossSim(HL.HostSim):
    """hostsim_lib.HostSim on the cross harness: step(T) runs the assemble step and the CROSS core, and keeps Cov(x_T), K, the window
    arrays and the two cross arrays ([B][N - 1][ns][ns] and [B][N][ns][ns], pre-filled with FILL)"""

    def __init__(self, params, batch):
        self.p, self.B, self.L = params, batch, cross_lib()
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.cov = self.xw = self.cw = self.l1 = self.zn = None
        self.K = 0

    def step(self, T):
        self.L.hs_ekf_step(self.h)
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        ns, N = self.p.dim_state, self.p.N
        self.cov = np.zeros((self.B, ns, ns))
        self.xw, self.cw = np.full((self.B, N, ns), FILL), np.full((self.B, N, ns, ns), FILL)
        self.l1, self.zn = np.full((self.B, N - 1, ns, ns), FILL), np.full((self.B, N, ns, ns), FILL)
        self.L.hs_update_direct_cross(self.h, T, HL._p(self.cov), HL._p(self.xw), HL._p(self.cw), HL._p(self.l1), HL._p(self.zn))
        self.K = min(T + 1, N)


def run_cross_sim(p, s, B, K, ticks):
    sim = CrossSim(p, B)
    out = {}
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k in ticks:
            M, n = sim.arrival()
            out[k] = dict(sim.get(), cov=sim.cov.copy(), M=M, n=n, K=sim.K, xw=sim.xw.copy(), cw=sim.cw.copy(), l1=sim.l1.copy(),
                          zn=sim.zn.copy())
    return out


def check_identities(g, b):
    """what holds to the bit inside one cross window, and what stays unwritten"""
    Kw = g["K"]
    assert np.array_equal(g["zn"][b, Kw - 1], g["cw"][b, Kw - 1])     # Z_{K-1} = P_{K-1}
    assert np.array_equal(g["zn"][b, Kw - 2], g["l1"][b, Kw - 2])     # Z_{K-2} = T1' P_{K-1} = W_{K-2}: one product, the same operands
    assert (g["l1"][b, Kw - 1:] == FILL).all() and (g["zn"][b, Kw:] == FILL).all()
    assert np.isfinite(g["l1"][b, :Kw - 1]).all() and np.isfinite(g["zn"][b, :Kw]).all()


@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_every_cross_block_is_a_block_of_the_kkt_inverse(name):
    mk, B, K, ticks = CORE_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    got = run_cross_sim(p, s, B, K, set(ticks))
    smooth = run_smooth_sim(p, s, B, K, set(ticks))
    N = p.N
    own_arrival = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    worst_1, worst_n, vo_eq = 0.0, 0.0, 0
    for b in range(B):
        arrival = {k: (got[k]["M"][b], got[k]["n"][b]) for k in ticks if k >= N} if own_arrival else None
        ref = cross_reference(p, s, b, set(ticks))
        ref_own = cross_reference(p, s, b, {k for k in ticks if k >= N}, arrival=arrival) if arrival else {}
        for k in ticks:
            Cf, nv = ref_own.get(k, ref[k])
            g, Kw = got[k], got[k]["K"]
            assert Kw == min(k + 1, N) == Cf.shape[0]
            assert g["status"][b] == capi.DEKF_SOLVE_OK
            # everything the SMOOTH core writes: the same bits, the unwritten tail included
            for key in ("x", "v_b", "status", "iters", "cov", "xw", "cw"):
                assert np.array_equal(g[key], smooth[k][key]), (k, key)
            check_identities(g, b)
            e1, en = cross_errors(g["l1"][b, :Kw - 1], g["zn"][b, :Kw], Cf)
            worst_1, worst_n, vo_eq = max(worst_1, e1), max(worst_n, en), vo_eq + nv
    print(f"[{name}] every cross block: worst lag-one error {worst_1:.3g}, worst to-newest error {worst_n:.3g} (units of "
          f"sqrt(Cov(x_a)_ii Cov(x_b)_jj)); VO equality rows in the checked windows: {vo_eq}")
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert worst_1 <= CREL
    assert worst_n <= CREL


@pytest.mark.parametrize("name,maker", [("go1", lambda: _params(go1_params)), ("cassie", lambda: _params(cassie_params))])
def test_core_without_vo_every_cross_block(name, maker):
    """no VO row (make_streams(vo=False)): the cross-covariances of the fixed-interval Kalman smoother on the window"""
    p = maker()
    B, K = 2, 2 * p.N + 5
    ticks = [3, p.N - 1, p.N, p.N + 7, K - 1]
    s = make_streams(p, B, K, vo=False)
    got = run_cross_sim(p, s, B, K, set(ticks))
    worst_1, worst_n = 0.0, 0.0
    for b in range(B):
        ref = cross_reference(p, s, b, set(ticks))
        for k in ticks:
            Cf, nv = ref[k]
            assert nv == 0
            Kw = got[k]["K"]
            check_identities(got[k], b)
            e1, en = cross_errors(got[k]["l1"][b, :Kw - 1], got[k]["zn"][b, :Kw], Cf)
            worst_1, worst_n = max(worst_1, e1), max(worst_n, en)
    print(f"[{name}, no VO] every cross block: worst lag-one error {worst_1:.3g}, worst to-newest error {worst_n:.3g}")
    assert worst_1 <= CREL
    assert worst_n <= CREL


def test_relative_cov_is_the_covariance_of_the_difference():
    """relative_cov on the reference's own blocks of one full go1 window against Cov(x_T - x_k) = D Cov D' formed from the full inverse
    (D = [.. -I .. I]); the cancellation is against the marginals, so the error is stated in the marginals' scale, as CREL is"""
    p = _params(go1_params)
    B, K = 1, 48
    s = rough_streams(p, B, K)
    (Cf, nv), = cross_reference(p, s, 0, {K - 1}).values()
    Kw, ns = Cf.shape[0], p.dim_state
    assert Kw == p.N and nv > 0
    cov_win = np.array([Cf[k, k] for k in range(Kw)])
    cov_newest = np.array([Cf[k, Kw - 1] for k in range(Kw)])
    full = Cf.transpose(0, 2, 1, 3).reshape(Kw * ns, Kw * ns)
    worst = 0.0
    for k in range(Kw):
        D = np.zeros((ns, Kw * ns))
        D[:, (Kw - 1) * ns:] += np.eye(ns)
        D[:, k * ns:(k + 1) * ns] -= np.eye(ns)
        want = D @ full @ D.T
        got = relative_cov(cov_win, cov_newest, k)
        dT, dk = np.sqrt(np.diagonal(Cf[Kw - 1, Kw - 1])), np.sqrt(np.diagonal(Cf[k, k]))
        scale = np.maximum(dT, dk)
        worst = max(worst, float((np.abs(got - want) / (scale[:, None] * scale[None, :])).max()))
    print(f"relative_cov against D Cov D' over one go1 window: worst {worst:.3g} of the marginals' scale")
    assert worst <= CREL
    # a batch axis in front works the same
    assert np.array_equal(relative_cov(cov_win[None], cov_newest[None], 3)[0], relative_cov(cov_win, cov_newest, 3))


ASAN_DRIVER = r"""
#include "direct_cross_hostsim.cpp"
#include <cmath>
#include <cstdio>
// synthetic sensors as in test_direct_smoother.py's driver, VO on every sixth step: window fill, marginalisation and VO rows.  All four
// window buffers are allocated at exactly their contract sizes ([B][N][...], lag-one [B][N-1][...]) and the guard behind the written
// entries is checked, so that an index past the window is caught by the sanitizer or by the guard.
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 2;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns);
    std::vector<int> mask(B, 1); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    int bad = 0;
    std::vector<double> xw, cw, l1, zn;
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
        l1.assign((size_t)B * (N - 1) * ns * ns, -7.0);
        zn.assign((size_t)B * N * ns * ns, -7.0);
        hs_update_direct_cross(h, T, cov.data(), xw.data(), cw.data(), l1.data(), zn.data());
        const int K = T + 1 < N ? T + 1 : N;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < N; ++k) {
                for (int i = 0; i < ns; ++i) { const double v = xw[((size_t)b * N + k) * ns + i]; bad += k < K ? !std::isfinite(v) : v != -7.0; }
                for (int i = 0; i < ns * ns; ++i) {
                    const double v = cw[((size_t)b * N + k) * ns * ns + i], z = zn[((size_t)b * N + k) * ns * ns + i];
                    bad += k < K ? !std::isfinite(v) : v != -7.0;
                    bad += k < K ? !std::isfinite(z) : z != -7.0;
                    if (k < N - 1) { const double w = l1[((size_t)b * (N - 1) + k) * ns * ns + i]; bad += k < K - 1 ? !std::isfinite(w) : w != -7.0; }
                }
            }
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d v=%g lag1=%g newest=%g, %d bad window entries\n", L, nj, N, ft,
                form, st[0], x[3], l1[0], zn[0], bad);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && bad == 0 ? 0 : 2;
}
int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }
"""


def test_cross_core_clean_under_asan_ubsan(tmp_path):
    """the CROSS core under AddressSanitizer + UBSan (CPU build): Go1 and foot states (both arrival-cost forms) through window fill,
    marginalisation and VO rows, the four window buffers exactly as large as the contract says"""
    src = tmp_path / "cross_driver.cpp"
    src.write_text(ASAN_DRIVER)
    exe = tmp_path / "cross_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
