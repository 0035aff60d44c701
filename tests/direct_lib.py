"""What the direct-solve tests share (test_direct_{solve,smoother,cross}.py and test_gpu_direct_{solve,smoother,cross}.py): the yardsticks,
the kernel catalogue, the error measures, the oracle reference (the exact optimum of the window QP and the inverse of its KKT matrix),
the checks of the C boundary, the lane-sequential harness (tests/hostsim/direct_hostsim.cpp) and the GPU runners.  The three variants
are named plain (the direct solve), smooth (with the window smoother) and cross (with the window cross-covariances on top).
TEST INFRASTRUCTURE ONLY.  Importing this module does not touch the GPU: torch and the estimator are imported where they are used."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import hostsim_lib as HL
import oracle_lib as O
import ref_numpy as RN
from decentralized_ekf_mhe_amd import capi, cassie_params, go1_params, pogox_params
from decentralized_ekf_mhe_amd.params import DekfParams
from decentralized_ekf_mhe_amd.streams import make_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decentralized_ekf_mhe_amd", "csrc")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
# exactness target per 3-block: |x - x*|_inf <= XREL |x*|_inf + XABS (the ADMM yardstick is 1e-4 / 1e-6)
XREL, XABS = 1e-8, 1e-10
# covariance: |C - C*|_ij <= CREL sqrt(C*_ii C*_jj)
CREL = 1e-7
FILL = -12345.0   # what the window buffers hold before an update: entries k >= K must keep it
# variant: the options of BatchedEstimator(solver="direct") and of run()
VARIANTS = {"plain": dict(smoother=False, cross=False), "smooth": dict(smoother=True, cross=False), "cross": dict(smoother=True, cross=True)}
# the direct kernels (name, L, leg_odom_type); every one has a _smooth and a _smooth_cross twin
KERNELS = [("k_mhe_solve_direct_4_n20", 4, 0), ("k_mhe_solve_direct_2_n20", 2, 0)] + \
    [(f"k_mhe_solve_direct_{L}", L, 0) for L in (1, 2, 3, 4)] + [(f"k_mhe_solve_direct_foot_{L}", L, 1) for L in (1, 2, 3, 4)]
LDS_BYTES, LDS_GRANULE = 160 * 1024, 1536


def direct_lds_bytes(ns):
    """the dynamic LDS of one workgroup of a direct kernel (mhe_direct_core.h: DirectScratch::len doubles)"""
    return (5 * ns * ns + 6 * ns + 8) * 8


def lds_workgroups_per_cu(ns):
    return LDS_BYTES // ((direct_lds_bytes(ns) + LDS_GRANULE - 1) // LDS_GRANULE * LDS_GRANULE)


# ------------------------------------------------------------------ shapes and streams
def _params(maker, **kw):
    p = maker()
    p.ekf_rate = p.rate
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def tripod_params(**kw):
    """3 legs x 6 joints at N = 12: no fixed-horizon kernel, the generic family solves every tick"""
    p = _params(go1_params, N=12, **kw)
    p.num_legs, p.joints_per_leg = 3, 6
    return p


def rough_streams(p, B, K, seed_shift=0):
    """make_streams logs with VO, camera drop-outs, a slow late camera on half the fleet and a flight phase longer than the window"""
    s = make_streams(p, B, K, first_instance=seed_shift, vo_rate=30.0)
    slow = make_streams(p, B, K, first_instance=seed_shift, vo_rate=3.75, vo_latency=0.06)
    half = np.arange(B) % 2 == 1
    for key in ("vo_mask", "vo_t_pre", "vo_t_now", "vo_dp", "vo_t_pose", "vo_q"):
        s[key][:, half] = slow[key][:, half]
    s["vo_any"] = s["vo_mask"].any(axis=1)
    L = p.num_legs
    f0, f1 = min(22, K - 1), min(22 + p.N + 4, K)
    s["contact"][f0:f1, ::3] = 0.0                        # every third robot in flight for longer than the window
    d0, d1 = min(30, K - 1), min(45, K)
    s["vo_mask"][d0:d1, 1::4] = 0                         # a camera drop-out on every fourth robot
    s["vo_any"] = s["vo_mask"].any(axis=1)
    assert s["contact"].shape[-1] == L
    return s


def sub_streams(s, idx, B):
    so = {k: (np.ascontiguousarray(v[:, idx]) if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == B else v) for k, v in s.items()}
    so["vo_any"] = so["vo_mask"].any(axis=1)
    return so


# ------------------------------------------------------------------ error measures
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


def window_errors(xw, cw, X, Cv, ns):
    """worst x error (units of the yardstick) and covariance error over the blocks of one window, and the block of the worst x error"""
    ex = [block_err(xw[j], X[j], blocks3(ns), XREL, XABS) for j in range(len(X))]
    ec = [cov_err(cw[j], Cv[j]) for j in range(len(X))]
    return max(ex), max(ec), int(np.argmax(ex))


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


# ------------------------------------------------------------------ the oracle reference
def kkt_of_qp(p, qp, k, arrival=None, solve=True, invert=True):
    """(x, Ki, xo, VO equality rows) of the window QP `qp` (Est.qp()) of an estimator at its step k >= 1: x the exact optimum
    (kkt_exact; None without `solve`), Ki the inverse of the KKT matrix, equilibrated as kkt_exact does (its (1, 1) block is the
    covariance of the window's variables; None without `invert`), xo the offsets of the K window states in both, oldest first
    (SURVEY.md Appendix A), and how many of the window's VO rows are equalities.
    arrival: (M_p, n_p) put in place of the oracle's arrival cost on the first block (1/2 x'M_p x + n_p'x)"""
    ns, nm = p.dim_state, 3 * p.num_legs
    sv = 2 * ns + nm + 3
    H, g, A, l, u = qp
    if arrival is not None:
        H, g = H.copy(), g.copy()
        H[:ns, :ns], g[:ns] = arrival
    n = H.shape[0]
    K = (n - ns - nm) // sv + 1
    assert K == min(k + 1, p.N) and (ns + nm) + (K - 1) * sv == n
    xo = [0 if j == 0 else (ns + nm) + (j - 1) * sv + ns + 3 for j in range(K)]
    assert xo[K - 1] == n - ns - nm
    x = RN.kkt_exact(H, g, A, l, u)[0] if solve else None
    Ki = None
    if invert:
        eq = (u - l) < 1e-9
        Ae = A[eq]
        KK = np.zeros((n + Ae.shape[0],) * 2)
        KK[:n, :n], KK[:n, n:], KK[n:, :n] = H, Ae.T, Ae
        d = 1.0 / np.sqrt(np.maximum(np.abs(KK).max(axis=1), 1e-300))
        Ki = np.linalg.inv(KK * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
    return x, Ki, xo, vo_equalities(p, A, l)


def kkt_reference(p, s, b, ticks, arrival=None, solve=True, invert=True):
    """Instance b through the oracle's pipe; at every tick in `ticks` yields (tick, x, Ki, xo, VO equality rows): kkt_of_qp of the
    oracle's window QP at that tick.  arrival: {tick: (M_p, n_p)} put in place of the oracle's arrival cost"""
    pipe = O.Pipe(p)
    for k in range(max(ticks) + 1):
        pipe.feed(s, k, b)
        pipe.step(k)
        if k not in ticks:
            continue
        yield (k,) + kkt_of_qp(p, pipe.est.qp(), k, None if arrival is None else arrival[k], solve, invert)


def exact_reference(p, s, b, ticks, cov=True, arrival=None):
    """{tick: (x_T, Cov(x_T), VO equality rows)} of instance b: the newest state of kkt_reference's optimum and its block of the inverse"""
    ns = p.dim_state
    return {k: (x[xo[-1]:xo[-1] + ns].copy(), Ki[xo[-1]:xo[-1] + ns, xo[-1]:xo[-1] + ns].copy() if cov else None, nv)
            for k, x, Ki, xo, nv in kkt_reference(p, s, b, ticks, arrival, invert=cov)}


def window_reference(p, s, b, ticks, arrival=None):
    """{tick: (x [K][ns], Cov [K][ns][ns], VO equality rows)} of instance b: the state blocks of kkt_reference's optimum and the diagonal
    state blocks of the inverse (exact_reference for every block)"""
    ns = p.dim_state
    return {k: (np.array([x[o:o + ns] for o in xo]), np.array([Ki[o:o + ns, o:o + ns] for o in xo]), nv)
            for k, x, Ki, xo, nv in kkt_reference(p, s, b, ticks, arrival)}


def cross_reference(p, s, b, ticks, arrival=None):
    """{tick: (Cov [K][K][ns][ns], VO equality rows)} of instance b: EVERY state block pair (a, c) -> Cov(x_a, x_c) of kkt_reference's
    inverse (window_reference extended to all index pairs)"""
    ns = p.dim_state
    out = {}
    for k, _, Ki, xo, nv in kkt_reference(p, s, b, ticks, arrival, solve=False):
        idx = np.concatenate([np.arange(o, o + ns) for o in xo])
        out[k] = (Ki[np.ix_(idx, idx)].reshape(len(xo), ns, len(xo), ns).transpose(0, 2, 1, 3).copy(), nv)
    return out


# ------------------------------------------------------------------ the C boundary
def header():
    return open(os.path.join(ROOT, "include", "dekf.h")).read()


def check_exports_and_binding(symbols):
    lib = capi.load()
    for name in symbols:
        assert hasattr(lib, name), name
        assert name in capi.PROTOTYPES, name


def check_abi_version_and_params_layout():
    lib = capi.load()
    assert lib.dekf_abi_version() == capi.DEKF_ABI_VERSION == 4
    p = DekfParams()
    lib.dekf_default_params(C.byref(p))
    assert bytes(p) == bytes(go1_params())


def check_c99_client(tmp_path, name, body, expect):
    """a C99 client of include/dekf.h whose main is `body` compiles without a warning, links, runs and prints `expect`"""
    src = tmp_path / (name + ".c")
    src.write_text('#include <stdio.h>\n#include "dekf.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-ldekf", f"-Wl,-rpath,{CSRC}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert expect in out.stdout, out.stdout


# variant: the robot_params members the shim sets, and what it prints in front of the print that closes every output line.  plain: C_MHE_
# behind every line's 9 + 3 columns; smooth: behind that window_steps_, then x_window_ and C_window_ of every window step; cross: behind
# the 9 + 3 columns window_steps_, then C_window_, C_newest_ and (but for the newest step) C_lag1_ of every window step
SHIM_PATCHES = {
    "plain": (["directSolve_"],
              "        for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_MHE_(i / 9, i % 9));\n"),
    "smooth": (["directSolve_", "smoothWindow_"],
               "        for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_MHE_(i / 9, i % 9));\n"
               "        std::printf(\" %d\", mhe.window_steps_);\n"
               "        for (int k = 0; k < mhe.window_steps_; ++k) {\n"
               "            for (int i = 0; i < 9; ++i) std::printf(\" %.17g\", mhe.x_window_[(size_t)k](i));\n"
               "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_window_[(size_t)k](i / 9, i % 9));\n"
               "        }\n"),
    "cross": (["directSolve_", "smoothWindow_", "windowCross_"],
              "        std::printf(\" %d\", mhe.window_steps_);\n"
              "        if (mhe.C_newest_.size() != (size_t)mhe.window_steps_) return 3;\n"
              "        if (mhe.window_steps_ > 0 && mhe.C_lag1_.size() + 1 != mhe.C_newest_.size()) return 3;\n"
              "        for (int k = 0; k < mhe.window_steps_; ++k) {\n"
              "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_window_[(size_t)k](i / 9, i % 9));\n"
              "            for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_newest_[(size_t)k](i / 9, i % 9));\n"
              "            if (k + 1 < mhe.window_steps_)\n"
              "                for (int i = 0; i < 81; ++i) std::printf(\" %.17g\", mhe.C_lag1_[(size_t)k](i / 9, i % 9));\n"
              "        }\n"),
}


def build_shim(tmp_path, variant):
    """examples/go1_shim_demo.cpp with the variant's SHIM_PATCHES applied, built in tmp_path"""
    flags, prints = SHIM_PATCHES[variant]
    src = open(os.path.join(ROOT, "examples", "go1_shim_demo.cpp")).read()
    src = src.replace('#include "../decentralized_ekf_mhe_amd/cpp/DecentralEst.hpp"',
                      '#include "' + os.path.join(ROOT, "decentralized_ekf_mhe_amd", "cpp", "DecentralEst.hpp") + '"')
    anchor = "    if (argc > 3) params->est_type_ = std::atoi(argv[3]);\n"
    assert anchor in src
    src = src.replace(anchor, anchor + "".join(f"    params->{f} = true;\n" for f in flags))
    anchor = '        std::printf(" %d\\n", mhe.solver_iters_);\n'
    assert anchor in src
    src = src.replace(anchor, prints + anchor)
    path = tmp_path / f"shim_{variant}.cpp"
    path.write_text(src)
    exe = str(tmp_path / f"shim_{variant}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", str(path), "-o", exe, "-L" + CSRC, "-ldekf",
                           "-Wl,-rpath," + CSRC, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def check_shim_usage(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def usage_table():
    """the product build's resource usage by kernel name (test_resource_usage.parse_usage), and the static LDS by kernel name"""
    from test_resource_usage import USAGE, _sources_mtime, parse_usage
    assert os.path.exists(USAGE) and os.path.getmtime(USAGE) >= _sources_mtime(), "build the library first (build.sh)"
    text = open(USAGE).read()
    static_lds = {blk.split("\n")[0].strip(): int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
                  for blk in text.split("Function Name: ")[1:]}
    return parse_usage(text), static_lds


def check_twins_at_their_design_point(sibling, twin):
    """every direct kernel's twin (suffix `twin`) against its sibling one option down (suffix `sibling`): no spills, no scratch, no
    static LDS, and an occupancy class not below the sibling's, or still above what the kernel's LDS admits"""
    table, static_lds = usage_table()
    for n, L, ft in KERNELS:
        assert n + sibling in table and n + twin in table, n
        u, t = table[n + sibling], table[n + twin]
        print(n + twin, t)
        assert t["spill"] == 0 and t["scratch"] == 0 and static_lds[n + twin] == 0, (n, t)
        lds_per_simd = lds_workgroups_per_cu(9 + 3 * L * ft) / 4.0
        assert t["occupancy"] >= u["occupancy"] or t["occupancy"] >= lds_per_simd, (n, t, u, lds_per_simd)


# the stand-alone sanitizer program: synthetic sensors as in test_hostsim_sanitizers.py, VO on every sixth step: window fill,
# marginalisation and VO rows.  A test gives the lines at the three marks: its buffers, its update with the checks of them (which count
# in `bad`), and its report line
ASAN_DRIVER = r"""
#include "direct_hostsim.cpp"
#include <cmath>
#include <cstdio>
static int run(int L, int nj, int N, int steps, int ft, int form) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.arrival_cost_form = form;
    const int ns = 9 + 3 * L * ft, B = 2;
    void* h = hs_create(&p, B);
    if (!h) return 1;
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B), cov((size_t)B * ns * ns);
    std::vector<int> mask(B, 1); std::vector<double> tp(B), tn(B), dp(3 * B), q(4 * B);
    int bad = 0;
    //BUFFERS
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
        //UPDATE
    }
    std::vector<double> x(ns * B); std::vector<int> st(B);
    hs_get(h, x.data(), nullptr, nullptr, nullptr, st.data(), nullptr, nullptr);
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d arrival_cost_form=%d: status %d v=%g ", L, nj, N, ft, form, st[0], x[3]);
    //REPORT
    hs_destroy(h);
    return st[0] == 1 && st[1] == 1 && bad == 0 ? 0 : 2;
}
int main() { return run(4, 3, 20, 50, 0, 0) | run(4, 3, 20, 34, 1, 0) | run(2, 5, 6, 24, 1, 1); }
"""


def check_clean_under_asan_ubsan(tmp_path, name, buffers, update, report):
    """ASAN_DRIVER with the test's lines, built with AddressSanitizer + UBSan (CPU build; test_hostsim_sanitizers.py does the same for
    the other cores) and run: Go1 and foot states (both arrival-cost forms)"""
    src = tmp_path / (name + ".cpp")
    src.write_text(ASAN_DRIVER.replace("//BUFFERS", buffers).replace("//UPDATE", update).replace("//REPORT", report))
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-w", "-I", HOSTSIM, "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------ the lane-sequential harness
LIB = os.path.join(HOSTSIM, "libdirect_hostsim.so")
_libs = {}


def direct_hostsim():
    """tests/hostsim/direct_hostsim.cpp as libdirect_hostsim.so, rebuilt when a source is newer, and bound"""
    if "lib" not in _libs:
        srcs = [os.path.join(HOSTSIM, f) for f in ("hostsim.cpp", "direct_hostsim.cpp")] + \
            [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-DDEKF_HOSTSIM", "-w", "-O2", "-o", LIB,
                                   os.path.join(HOSTSIM, "direct_hostsim.cpp")])
        L = HL._bind(C.CDLL(LIB))
        L.hs_update_direct.argtypes = [C.c_void_p, C.c_int, HL._dp]
        L.hs_update_direct_smooth.argtypes = [C.c_void_p, C.c_int, HL._dp, HL._dp, HL._dp]
        L.hs_update_direct_cross.argtypes = [C.c_void_p, C.c_int, HL._dp, HL._dp, HL._dp, HL._dp, HL._dp]
        _libs["lib"] = L
    return _libs["lib"]


class DirectSim(HL.HostSim):
    """hostsim_lib.HostSim on the direct harness: step(T) runs the assemble step and the variant's core, and keeps Cov(x_T) and, of a
    smooth or cross variant, K and in `win` the window arrays xw, cw ([B][N][...]); of a cross variant the cross arrays l1
    ([B][N - 1][ns][ns]) and zn ([B][N][ns][ns]) too.  The arrays of `win` are pre-filled with FILL"""

    def __init__(self, params, batch, variant="plain"):
        assert variant in VARIANTS
        self.p, self.B, self.L, self.variant = params, batch, direct_hostsim(), variant
        self.h = self.L.hs_create(C.byref(params), batch)
        assert self.h, "hs_create rejected the parameters"
        self.cov = None
        self.win = {}
        self.K = 0

    def ekf_step(self):
        self.L.hs_ekf_step(self.h)

    def step(self, T):
        self.ekf_step()
        self.update(T)

    def update(self, T):
        """the MHE timer's event alone: hs_initialize at T = 0, else the variant's update"""
        if T == 0:
            self.L.hs_initialize(self.h)
            return
        ns, N, B = self.p.dim_state, self.p.N, self.B
        self.cov = np.zeros((B, ns, ns))
        if self.variant == "plain":
            self.L.hs_update_direct(self.h, T, HL._p(self.cov))
            return
        self.win = dict(xw=np.full((B, N, ns), FILL), cw=np.full((B, N, ns, ns), FILL))
        if self.variant == "smooth":
            self.L.hs_update_direct_smooth(self.h, T, HL._p(self.cov), HL._p(self.win["xw"]), HL._p(self.win["cw"]))
        else:
            self.win.update(l1=np.full((B, N - 1, ns, ns), FILL), zn=np.full((B, N, ns, ns), FILL))
            self.L.hs_update_direct_cross(self.h, T, HL._p(self.cov), *(HL._p(self.win[k]) for k in ("xw", "cw", "l1", "zn")))
        self.K = min(T + 1, N)


def run_direct_sim(p, s, B, K, ticks, variant="plain"):
    """{tick: what the variant's core left}: hostsim_lib.HostSim.get()'s keys, cov, the arrival cost M, n and, but for plain, K and
    DirectSim's window arrays"""
    sim = DirectSim(p, B, variant)
    out = {}
    for k in range(K):
        sim.feed(s, k)
        sim.step(k)
        if k in ticks:
            M, n = sim.arrival()  # (the arrival cost this tick's solve read: the update runs the assemble step in place)
            out[k] = dict(sim.get(), cov=sim.cov.copy(), M=M, n=n)
            if variant != "plain":
                out[k].update({key: a.copy() for key, a in sim.win.items()}, K=sim.K)
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


def own_arrival(p, got, ticks, b):
    """{tick: (M_p, n_p)} of the full windows of a lane-sequential run `got`, where the case is held against its own arrival cost
    (CORE_CASES: arrival_cost_form 1); None elsewhere"""
    if not (p.leg_odom_type == 1 and p.arrival_cost_form == 1):
        return None
    return {k: (got[k]["M"][b], got[k]["n"][b]) for k in ticks if k >= p.N}


# ------------------------------------------------------------------ the GPU runners
def run(p, s, B, K, solver="direct", smoother=False, cross=False, every=1, reset_rerun=False, keep=None):
    """x, v_b, status, iters, residuals and (direct) Cov(x_T) at the read ticks (every `every`-th tick and the last); of a smoothing
    handle the window too (K, xw, cw of the instances `keep`, default all) and of a cross handle the cross-covariances (l1, zn), as
    lists over the read ticks from tick 1 on"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    est = BatchedEstimator(p, B, solver=solver, smoother=smoother, cross=cross)
    sh = streams_host(s)
    keep = list(range(B)) if keep is None else keep
    res = []
    lists = ("xw", "cw", "l1", "zn")
    for _ in range(2 if reset_rerun else 1):
        out = {k: [] for k in ("x", "vb", "st", "it", "pri", "cov", "ticks", "K") + lists}
        for k in range(K):
            est.push_stream_step(sh, k)
            est.step(k)
            if k % every == 0 or k == K - 1:
                o, info = est.get(), est.solver_info()
                out["x"].append(o["x"]); out["vb"].append(o["v_b"]); out["st"].append(o["status"]); out["it"].append(info["iters"])
                out["pri"].append(info["pri_res"]); out["ticks"].append(k)
                if solver == "direct" and k:
                    out["cov"].append(est.mhe_cov())
                if smoother and k:
                    Kw, xw, cw = est.window()
                    out["K"].append(Kw); out["xw"].append(xw[keep]); out["cw"].append(cw[keep])
                if cross and k:
                    Kc, l1, zn = est.window_cross()
                    assert Kc == Kw and l1.shape[1] == Kw - 1 and zn.shape[1] == Kw
                    out["l1"].append(l1[keep]); out["zn"].append(zn[keep])
        r = {k: (v if k in lists else np.array(v)) for k, v in out.items()}
        r["kernel"] = (est.solve_kernel_name(True), est.solve_kernel_name(False))
        res.append(r)
        if reset_rerun:
            est.reset()
    est.close()
    return res if reset_rerun else res[0]


# name: (params, B, K, oracle instances, every, direct kernel).  rough_streams: the even instances carry the 30 Hz camera, whose VO rows
# turn into equalities from tick 40 on (the odd ones the slow camera): every case runs past that and checks even and odd instances.
CASES = {
    "go1_832": (lambda: _params(go1_params), 832, 48, [0, 1, 416, 831], 1, "k_mhe_solve_direct_4_n20"),
    "cassie": (lambda: _params(cassie_params), 6, 48, [0, 3], 1, "k_mhe_solve_direct_2_n20"),
    "pogox_n100": (lambda: _params(pogox_params), 4, 111, [0, 1], 10, "k_mhe_solve_direct_1"),  # (KKT systems ~3 900 wide: every 10th tick)
    "tripod": (lambda: tripod_params(), 6, 48, [0, 5], 1, "k_mhe_solve_direct_3"),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 6, 48, [0, 1], 1, "k_mhe_solve_direct_foot_4"),
    "go1_foot_info": (lambda: _params(go1_params, leg_odom_type=1, arrival_cost_form=1), 4, 48, [2], 1, "k_mhe_solve_direct_foot_4"),
}
# the cross variant's: (params, B, ticks, instances checked, every, kernel).  The smallest shapes that take every path: Go1 is the _4_n20
# twin with the fast (even) and the slow (odd) camera; go1_foot has ns = 21, several entries per lane and the blocks that bound LDS;
# PogoX is the run-time horizon with a 99-step chain of Z.  The foot-state references are KKT systems ~2 200 wide (every 8th tick, which
# still takes the window fill, full windows and, from tick 40 on, VO equality rows), PogoX's ~3 900 wide (every 10th, one instance).
CROSS_CASES = {
    "go1": (lambda: _params(go1_params), 6, 48, [0, 1], 1, "k_mhe_solve_direct_4_n20"),
    "go1_foot": (lambda: _params(go1_params, leg_odom_type=1), 4, 48, [0, 1], 8, "k_mhe_solve_direct_foot_4"),
    "pogox_n100": (lambda: _params(pogox_params), 2, 111, [0], 10, "k_mhe_solve_direct_1"),
    "go1_foot_info": (lambda: _params(go1_params, leg_odom_type=1, arrival_cost_form=1), 2, 48, [0], 8, "k_mhe_solve_direct_foot_4"),
}


@functools.lru_cache(maxsize=None)
def case_run(name, variant):
    """(params, streams, kept instances, run) of a case of CASES (cross: of CROSS_CASES), once per process.  A smooth run keeps the
    windows of the oracle instances and of the first six, every other run those of all instances"""
    mk, B, K, sub, every, kernel = (CROSS_CASES if variant == "cross" else CASES)[name]
    p = mk()
    s = rough_streams(p, B, K)
    keep = sorted(set(sub) | set(range(min(B, 6)))) if variant == "smooth" else list(range(B))
    return p, s, keep, run(p, s, B, K, every=every, keep=keep, **VARIANTS[variant])


def check_reset_rerun(variant, keys=()):
    """a handle run, reset and run again gives the bits of a fresh handle both times: x, v_b, status, Cov(x_T), K and the window arrays
    `keys` of every read tick"""
    p = _params(go1_params)
    B, K = 8, 30
    s = rough_streams(p, B, K)
    a, b = run(p, s, B, K, every=3, reset_rerun=True, **VARIANTS[variant])
    fresh = run(p, s, B, K, every=3, **VARIANTS[variant])
    for other in (a, b):
        for key in ("x", "vb", "st", "cov", "K"):
            assert np.array_equal(other[key], fresh[key]), key
        for i in range(len(fresh["K"])):
            for key in keys:
                assert np.array_equal(other[key][i], fresh[key][i]), (key, i)


def poisoned_runs(variant, keys=()):
    """A NaN accelerometer sample on one instance at one tick (poisoned data, no fault): every other instance keeps the bits of the
    clean run in x, v_b, status, Cov(x_T) and the window arrays `keys`, which are finite throughout the clean run; the poisoned
    instance reports DEKF_SOLVE_NUMERIC at that tick, and wherever it does, its entries of `keys` are NaN throughout.
    Returns (params, poisoned streams, B, K, clean run, poisoned run)"""
    p = _params(go1_params)
    B, K, bad, t_bad = 6, 34, 2, 26
    s = rough_streams(p, B, K)
    clean = run(p, s, B, K, **VARIANTS[variant])
    sp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    sp["accel"][t_bad, bad, 0] = np.nan
    pois = run(p, sp, B, K, **VARIANTS[variant])
    others = [b for b in range(B) if b != bad]
    for key in ("x", "vb", "st", "cov"):
        assert np.array_equal(pois[key][:, others], clean[key][:, others]), key
    assert np.array_equal(pois["K"], clean["K"])
    assert (clean["st"][1:] == capi.DEKF_SOLVE_OK).all()
    assert pois["st"][t_bad, bad] == capi.DEKF_SOLVE_NUMERIC
    n_numeric = 0
    for i in range(len(clean["K"])):
        for key in keys:
            assert np.array_equal(pois[key][i][others], clean[key][i][others]), (key, i)
            assert np.isfinite(clean[key][i]).all(), (key, i)
        if pois["st"][i + 1, bad] == capi.DEKF_SOLVE_NUMERIC:     # (read tick i + 1: the window arrays start at tick 1)
            n_numeric += 1
            assert all(np.isnan(pois[key][i][bad]).all() for key in keys), i
    if keys:
        assert n_numeric >= 1
    return p, sp, B, K, clean, pois


def check_window_pointers(cross):
    """dekf_get_window (cross: dekf_get_window_cross) through the window fill and beyond: host and device pointers give the same bits,
    the entries past the written ones keep FILL, any of the three pointers may be NULL, and the Python accessor hands out the written
    entries.  The first array is x_win [B][N][ns] with K written entries (cross: cov_lag1 [B][N - 1][ns][ns] with K - 1), the second
    cov_win (cross: cov_newest) [B][N][ns][ns] with K"""
    import torch
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    lib = capi.load()
    get = lib.dekf_get_window_cross if cross else lib.dekf_get_window
    p = _params(go1_params)
    B, ns, N = 5, p.dim_state, p.N
    shape_a, shape_b = ((B, N - 1, ns, ns) if cross else (B, N, ns)), (B, N, ns, ns)
    s = rough_streams(p, B, N + 4)
    est = BatchedEstimator(p, B, solver="direct", smoother=True, cross=cross)
    sh = streams_host(s)
    for k in range(N + 4):
        est.push_stream_step(sh, k)
        est.step(k)
        if k not in (1, 7, N - 2, N - 1, N + 3):
            continue
        Kw = min(k + 1, N)
        Ka = Kw - 1 if cross else Kw
        ah, bh = np.full(shape_a, FILL), np.full(shape_b, FILL)
        kh = C.c_int(0)
        assert get(est.h, C.byref(kh), ah.ctypes.data, bh.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert kh.value == Kw
        assert (ah[:, Ka:] == FILL).all() and (bh[:, Kw:] == FILL).all(), k
        assert np.isfinite(ah[:, :Ka]).all() and np.isfinite(bh[:, :Kw]).all(), k
        ad = torch.full(shape_a, FILL, dtype=torch.float64, device="cuda")
        bd = torch.full(shape_b, FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        kd = C.c_int(0)
        assert get(est.h, C.byref(kd), ad.data_ptr(), bd.data_ptr(), capi.DEKF_DEVICE) == capi.DEKF_OK
        est.sync()
        assert kd.value == Kw
        assert np.array_equal(ad.cpu().numpy(), ah) and np.array_equal(bd.cpu().numpy(), bh), k
        # any of the three pointers may be NULL
        a2 = np.full(shape_a, FILL)
        assert get(est.h, None, a2.ctypes.data, None, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(a2, ah)
        b2 = np.full(shape_b, FILL)
        assert get(est.h, None, None, b2.ctypes.data, capi.DEKF_HOST) == capi.DEKF_OK
        assert np.array_equal(b2, bh)
        k3 = C.c_int(0)
        assert get(est.h, C.byref(k3), None, None, capi.DEKF_HOST) == capi.DEKF_OK and k3.value == Kw
        # window() / window_cross() hands out the written entries
        Kp, ap, bp = est.window_cross() if cross else est.window()
        assert Kp == Kw and np.array_equal(ap, ah[:, :Ka]) and np.array_equal(bp, bh[:, :Kw])
    est.close()


def shim_rows(exe, tmp_path, p, K):
    """One robot's make_streams log of K ticks, with the oracle's orientation, packed into the shim's 81-column log and run through the
    shim program `exe`: (streams, quaternions, the numbers of every output line behind the first)"""
    s = make_streams(p, 1, K)
    quats = O.run_streams(p, s)[2][:, 0]
    log = np.zeros((K, 81))
    for k in range(K):
        log[k, 0] = s["imu_t"][k, 0]
        log[k, 1:4], log[k, 4:7], log[k, 7:11] = s["accel"][k, 0], s["gyro"][k, 0], quats[k]
        log[k, 11:23] = s["p_foot"][k, 0].ravel()
        log[k, 23:59] = s["J"][k, 0].ravel()
        log[k, 59:71] = s["qdot"][k, 0].ravel()
        log[k, 71:75] = s["contact"][k, 0]
        if s["vo_mask"][k, 0]:
            log[k, 75], log[k, 76], log[k, 77], log[k, 78:81] = 1.0, s["vo_t_pre"][k, 0], s["vo_t_now"][k, 0], s["vo_dp"][k, 0]
    path = tmp_path / "log.bin"
    log.tofile(path)
    r = subprocess.run([exe, str(path), str(K)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return s, quats, [np.array([float(v) for v in line.split()[1:]]) for line in r.stdout.strip().splitlines()]


def shim_twin(p, s, quats, K, variant):
    """the same robot through BatchedEstimator, with the orientation the shim was given: yields (tick, estimator) after every update"""
    from decentralized_ekf_mhe_amd.estimator import BatchedEstimator, streams_host
    est = BatchedEstimator(p, 1, solver="direct", **VARIANTS[variant])
    sh = streams_host(s)
    for k in range(K):
        est.push_stream_step(sh, k)
        est.push_quaternion(np.ascontiguousarray(quats[k][None, :]))
        est.update(k) if k else est.initialize()
        if k:
            yield k, est
    est.close()
