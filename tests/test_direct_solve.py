"""The direct MHE solve (dekf_set_solver(h, DEKF_SOLVER_DIRECT), csrc/mhe_direct_core.h) without a GPU.

ABI: the two calls are declared, exported and bound, refuse a null handle and compile as C99, while the ABI version and dekf_params
stay what they were; the C++ shim compiles with robot_params::directSolve_ and C_MHE_; the direct kernels sit at their design point.
Core: the lane-sequential build of the direct core (tests/hostsim/direct_hostsim.cpp) on the records and the input snapshot that the
assemble step leaves, every checked tick against the exact optimum of the oracle's QP (ref_numpy.kkt_exact) and the covariance of
x_T against the inverse of that QP's KKT matrix; without VO against the numpy Kalman filter (KA1)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hostsim_lib as HL
import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params, pogox_params
from decentralized_ekf_mhe_amd.params import DekfParams
from decentralized_ekf_mhe_amd.streams import make_streams
from test_gpu_warm_start import _params, rough_streams, tripod_params  # (the shapes and streams of the warm-start tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decentralized_ekf_mhe_amd", "csrc")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
SYMBOLS = ("dekf_set_solver", "dekf_get_mhe_cov")
# exactness target per 3-block: |x - x*|_inf <= XREL |x*|_inf + XABS (the ADMM yardstick is 1e-4 / 1e-6)
XREL, XABS = 1e-8, 1e-10
# covariance: |C - C*|_ij <= CREL sqrt(C*_ii C*_jj)
CREL = 1e-7


def block_err(x, ref, blocks, rtol, atol):
    """worst over the blocks of |x - ref|_inf / (rtol |ref|_inf + atol)"""
    worst = 0.0
    for blk in blocks:
        num = np.abs(x[..., blk] - ref[..., blk]).max(axis=-1)
        den = rtol * np.abs(ref[..., blk]).max(axis=-1) + atol
        worst = max(worst, float(np.max(num / den)))
    return worst


def blocks3(ns):
    return [slice(i, i + 3) for i in range(0, ns, 3)]


def cov_err(Cm, Cref):
    d = np.sqrt(np.abs(np.diagonal(Cref, axis1=-2, axis2=-1)))
    return float((np.abs(Cm - Cref) / (d[..., :, None] * d[..., None, :])).max())


def vo_equalities(p, A, l):
    """VO rows of the window QP that hold as equalities (vision has written their bound): the VO rows are the last three of every
    step block [Meas | Dyn | VO] after the first Meas block, the free ones carry -1e30"""
    nm, ns = 3 * p.num_legs, p.dim_state
    sc = nm + ns + 3
    steps = (A.shape[0] - nm) // sc
    vo_rows = np.concatenate([nm + k * sc + ns + np.arange(3) for k in range(steps)]).astype(int)
    return int(np.sum(np.abs(l[vo_rows]) < 1e20))


def exact_reference(p, s, b, ticks, cov=True, arrival=None):
    """{tick: (x_T, Cov(x_T), VO equality rows)} of instance b: the exact optimum of the oracle's window QP (kkt_exact), the x_T block
    of the (1, 1) block of the inverse of its KKT matrix, equilibrated as kkt_exact does, and how many of the window's VO rows are
    equalities.  arrival: {tick: (M_p, n_p)} put in place of the oracle's arrival cost on the first block (1/2 x'M_p x + n_p'x)"""
    ns, nm = p.dim_state, 3 * p.num_legs
    pipe = O.Pipe(p)
    out = {}
    K = max(ticks) + 1
    for k in range(K):
        pipe.feed(s, k, b)
        pipe.step(k)
        if k not in ticks:
            continue
        H, g, A, l, u = pipe.est.qp()
        if arrival is not None:
            H, g = H.copy(), g.copy()
            H[:ns, :ns], g[:ns] = arrival[k]
        x, _ = RN.kkt_exact(H, g, A, l, u)
        n = H.shape[0]
        xs = slice(n - ns - nm, n - nm)
        Cr = None
        if cov:
            eq = (u - l) < 1e-9
            Ae = A[eq]
            KK = np.zeros((n + Ae.shape[0],) * 2)
            KK[:n, :n], KK[:n, n:], KK[n:, :n] = H, Ae.T, Ae
            d = 1.0 / np.sqrt(np.maximum(np.abs(KK).max(axis=1), 1e-300))
            Ki = np.linalg.inv(KK * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
            Cr = Ki[xs, xs]
        out[k] = (x[xs].copy(), Cr, vo_equalities(p, A, l))
    return out


# ------------------------------------------------------------------ 1: the C boundary
def _header():
    return open(os.path.join(ROOT, "include", "dekf.h")).read()


def test_header_declares_both_calls_and_the_solver_values():
    hdr = _header()
    assert re.search(r"dekf_status\s+dekf_set_solver\s*\(\s*dekf_handle\s+h\s*,\s*int\s+solver\s*\)\s*;", hdr)
    assert re.search(r"dekf_status\s+dekf_get_mhe_cov\s*\(\s*dekf_handle\s+h\s*,\s*double\s*\*\s*cov\s*,\s*dekf_mem\s+where\s*\)\s*;", hdr)
    assert re.search(r"#define\s+DEKF_SOLVER_ADMM\s+0\b", hdr) and re.search(r"#define\s+DEKF_SOLVER_DIRECT\s+1\b", hdr)
    assert (capi.DEKF_SOLVER_ADMM, capi.DEKF_SOLVER_DIRECT) == (0, 1)


def test_library_exports_and_binding_lists_them():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name
    assert capi.PROTOTYPES["dekf_set_solver"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.PROTOTYPES["dekf_get_mhe_cov"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])


def test_abi_version_and_params_layout_unchanged():
    lib = capi.load()
    assert lib.dekf_abi_version() == capi.DEKF_ABI_VERSION == 4
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    assert bytes(p) == bytes(go1_params())


def test_null_handle_is_invalid():
    lib = capi.load()
    for solver in (0, 1, 2):
        assert lib.dekf_set_solver(None, solver) == capi.DEKF_ERR_INVALID
    cov = (C.c_double * 81)()
    assert lib.dekf_get_mhe_cov(None, C.cast(cov, C.c_void_p), capi.DEKF_HOST) == capi.DEKF_ERR_INVALID


def test_header_compiles_as_c99_with_the_direct_calls(tmp_path):
    src = tmp_path / "direct_client.c"
    src.write_text(
        '#include <stdio.h>\n#include "dekf.h"\n'
        "int main(void) {\n"
        "    double cov[81];\n"
        "    dekf_status a = dekf_set_solver((dekf_handle)0, DEKF_SOLVER_DIRECT);\n"
        "    dekf_status b = dekf_get_mhe_cov((dekf_handle)0, cov, DEKF_HOST);\n"
        '    printf("set %d get %d admm %d\\n", (int)a, (int)b, DEKF_SOLVER_ADMM);\n'
        "    return 0;\n}\n")
    exe = tmp_path / "direct_client"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-ldekf", f"-Wl,-rpath,{CSRC}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert f"set {capi.DEKF_ERR_INVALID} get {capi.DEKF_ERR_INVALID} admm 0" in out.stdout, out.stdout


def shim_direct_source():
    """examples/go1_shim_demo.cpp with robot_params::directSolve_ set and C_MHE_ printed behind every line"""
    src = open(os.path.join(ROOT, "examples", "go1_shim_demo.cpp")).read()
    src = src.replace('#include "../decentralized_ekf_mhe_amd/cpp/DecentralEst.hpp"',
                      '#include "' + os.path.join(ROOT, "decentralized_ekf_mhe_amd", "cpp", "DecentralEst.hpp") + '"')
    anchor = "    if (argc > 3) params->est_type_ = std::atoi(argv[3]);\n"
    assert anchor in src
    src = src.replace(anchor, anchor + "    params->directSolve_ = true;\n")
    anchor = '        std::printf(" %d\\n", mhe.solver_iters_);\n'
    assert anchor in src
    src = src.replace(anchor, "        for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_MHE_(i / 9, i % 9));\n" + anchor)
    return src


def build_shim_direct(tmp_path):
    src = tmp_path / "shim_direct.cpp"
    src.write_text(shim_direct_source())
    exe = str(tmp_path / "shim_direct")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", str(src), "-o", exe, "-L" + CSRC, "-ldekf",
                           "-Wl,-rpath," + CSRC, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_compiles_with_direct_solve_and_its_covariance(tmp_path):
    exe = build_shim_direct(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_direct_kernels_at_their_design_point():
    """one wavefront per instance, no spills, <= 72 VGPRs (>= 7 wavefronts per SIMD as far as registers go), and
    LDS for at least 8 workgroups per CU (2 wavefronts per SIMD: the dynamic LDS, which the compiler's occupancy figure does not see)"""
    from test_resource_usage import USAGE, _sources_mtime, parse_usage
    assert os.path.exists(USAGE) and os.path.getmtime(USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    table = parse_usage(open(USAGE).read())
    names = [f"k_mhe_solve_direct_{s}" for s in ("4_n20", "2_n20", "1", "2", "3", "4", "foot_1", "foot_2", "foot_3", "foot_4")]
    for n in names:
        assert n in table, n
        u = table[n]
        assert u["spill"] == 0 and u["scratch"] == 0 and u["vgprs"] + (u["agprs"] or 0) <= 72 and u["occupancy"] >= 7, (n, u)
    for L in range(1, 5):  # the largest state of each leg count: 9 + 3 L with foot positions (mhe_direct_core.h: DirectScratch)
        ns = 9 + 3 * L
        lds = (5 * ns * ns + 6 * ns + 8) * 8
        granule = 1536
        assert (160 * 1024) // ((lds + granule - 1) // granule * granule) >= 8, (L, lds)


# ------------------------------------------------------------------ 2: the core, lane-sequential
LIB = os.path.join(HOSTSIM, "libdirect_hostsim.so")


def build_direct_hostsim():
    srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                               os.path.join(HOSTSIM, "direct_hostsim.cpp")])
    return LIB


_libs = {}


def direct_lib():
    if "lib" not in _libs:
        L = HL._bind(C.CDLL(build_direct_hostsim()))
        L.hs_update_direct.argtypes = [C.c_void_p, C.c_int, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


class DirectSim(HL.HostSim):
    """hostsim_lib.HostSim on the direct harness: step(T) runs the assemble step and the direct core, and keeps Cov(x_T)"""

    def __init__(self, params, batch):
        self.p, self.B, self.L = params, batch, direct_lib()
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.cov = None

    def step(self, T):
        self.L.hs_ekf_step(self.h)
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        ns = self.p.dim_state
        self.cov = np.zeros((self.B, ns, ns))
        self.L.hs_update_direct(self.h, T, HL._p(self.cov))


def run_direct_sim(p, s, B, K, ticks):
    sim = DirectSim(p, B)
    out = {}
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k in ticks:
            M, n = sim.arrival()  # (the arrival cost this tick's solve read: hs_update_direct runs the assemble step in place)
            out[k] = dict(sim.get(), cov=sim.cov.copy(), M=M, n=n)
    return out


# name: (params, B, K, ticks checked).  rough_streams: the even instances carry the 30 Hz camera, whose VO rows turn into equalities
# from tick 40 on (the odd ones the slow camera): every case runs past that, so that the checked windows hold VO equality rows.
CORE_CASES = {
    "go1": (lambda: _params(go1_params), 2, 48, list(range(1, 48, 3)) + [41, 44, 47]),
    "cassie": (lambda: _params(cassie_params), 2, 48, list(range(1, 48, 3)) + [41, 44, 47]),
    "pogox_n100": (lambda: _params(pogox_params), 1, 111, list(range(10, 111, 10))),
    "tripod": (lambda: tripod_params(), 2, 48, list(range(1, 48, 3)) + [41, 44, 47]),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 2, 48, list(range(1, 48, 3)) + [41, 44, 47]),
    # arrival_cost_form 1: the information-form arrival cost differs from the oracle's covariance form by rounding, so the full windows
    # are held against the oracle's QP with THIS solve's arrival cost in place (the solve exact; the arrival cost is another step's)
    "go1_foot_info": (lambda: _params(go1_params, leg_odom_type=1, arrival_cost_form=1), 1, 48, list(range(1, 48, 3)) + [41, 44, 47]),
}


@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_is_the_exact_optimum_of_the_oracle_qp(name):
    mk, B, K, ticks = CORE_CASES[name]
    p = mk()
    s = rough_streams(p, B, K)
    got = run_direct_sim(p, s, B, K, set(ticks))
    ns, N = p.dim_state, p.N
    own_arrival = p.leg_odom_type == 1 and p.arrival_cost_form == 1
    worst_x, worst_c, worst_fill, vo_eq = 0.0, 0.0, 0.0, 0
    for b in range(B):
        arrival = {k: (got[k]["M"][b], got[k]["n"][b]) for k in ticks if k >= N} if own_arrival else None
        ref = exact_reference(p, s, b, set(ticks))
        ref_own = exact_reference(p, s, b, {k for k in ticks if k >= N}, arrival=arrival) if arrival else {}
        for k in ticks:
            xr, Cr, nv = ref_own.get(k, ref[k])
            x, Cm = got[k]["x"][b], got[k]["cov"][b]
            assert got[k]["status"][b] == capi.DEKF_SOLVE_OK
            assert got[k]["iters"][b] == 0 and np.isnan(got[k]["pri_res"][b]) and np.isnan(got[k]["dua_res"][b])
            ex = block_err(x, xr, blocks3(ns), XREL, XABS)
            ec = cov_err(Cm, Cr)
            worst_x, worst_c, vo_eq = max(worst_x, ex), max(worst_c, ec), vo_eq + nv
            if k < N:
                worst_fill = max(worst_fill, ex)
    print(f"[{name}] worst x error {worst_x:.3g} x (1e-8 rel + 1e-10), window fill {worst_fill:.3g} x; worst covariance error "
          f"{worst_c:.3g} sqrt(C_ii C_jj); VO equality rows in the checked windows: {vo_eq}")
    assert vo_eq > 0, "no checked window holds a VO equality row"
    assert worst_x <= 1.0
    assert worst_c <= CREL


@pytest.mark.parametrize("name,maker", [("go1", lambda: _params(go1_params)), ("cassie", lambda: _params(cassie_params))])
def test_core_without_vo_is_the_kalman_filter(name, maker):
    """no VO row: the forward elimination is the Kalman filter on the window (KA1's identity; ref_numpy.kalman_filter with
    ref_double_init=False, as KA1 uses it)"""
    p = maker()
    B, K = 2, 3 * p.N + 5
    s = make_streams(p, B, K, vo=False)
    sim = DirectSim(p, B)
    xs, covs, quats = [], [], []
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        o = sim.get()
        quats.append(o["quat"].copy())
        if k:
            xs.append(o["x"].copy())
            covs.append(sim.cov.copy())
    quats = np.array(quats)
    for b in range(B):
        xk, Ck = RN.kalman_filter(p, s, b, quats[:, b])
        for k in range(1, K):
            for blk in blocks3(p.dim_state):
                rel = np.abs(xs[k - 1][b][blk] - xk[k][blk]).max() / max(np.abs(xk[k][blk]).max(), 1e-6)
                assert rel < 1e-7, (b, k, blk, rel)
            assert cov_err(covs[k - 1][b], Ck[k]) <= CREL, (b, k)


def test_core_against_the_cold_admm_oracle():
    """a record, not the pin: how far the reference's own ADMM output (the cold CPU oracle, eps 1e-6) lies from the exact optimum, every
    tick, in units of the ADMM yardstick (1e-4 rel + 1e-6 per 3-block); warm start measured 2.1 x / 8.3 x against the same oracle"""
    p = _params(go1_params)
    B, K = 2, 40
    s = rough_streams(p, B, K)
    got = run_direct_sim(p, s, B, K, set(range(1, K)))
    x_ref, _, _, _ = O.run_streams(p, s)
    x = np.array([got[k]["x"] for k in range(1, K)])
    e = block_err(x, x_ref[1:], blocks3(9), 1e-4, 1e-6)
    print(f"direct against the cold ADMM oracle: {e:.2f} x the yardstick")
    assert e <= 2.5   # (measured 1.06 x: the oracle's iterate in the first steps after VO rows switch on, cf. test_oracle_mhe.py KA2)


ASAN_DRIVER = r"""
#include "direct_hostsim.cpp"
#include <cstdio>
// synthetic sensors as in test_hostsim_sanitizers.py, VO on every sixth step: window fill, marginalisation and VO rows
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 2;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns);
    std::vector<int> mask(B, 1); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
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
        if (T == 0) hs_initialize(h); else hs_update_direct(h, T, cov.data());
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d v=%g cov00=%g\n", L, nj, N, ft, form, st[0], x[3], cov[0]);
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 ? 0 : 2;
}
int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }
"""


def test_core_clean_under_asan_ubsan(tmp_path):
    """the direct core under AddressSanitizer + UBSan (CPU build; test_hostsim_sanitizers.py does the same for the other cores): Go1
    and foot states (both arrival-cost forms) through window fill, marginalisation and VO rows"""
    src = tmp_path / "direct_driver.cpp"
    src.write_text(ASAN_DRIVER)
    exe = tmp_path / "direct_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
