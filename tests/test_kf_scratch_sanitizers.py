"""The Kalman-filter cores (kf_core.h, est_type 1) under AddressSanitizer + UBSan with exactly the scratch the device gives them.
hs_create sizes the lane-sequential build's scratch as the largest of the solve's, the assembly's and the filter's, so an overrun of
KfScratch::len would land in slack; the k_kf_* kernels get KfScratch::len(L, leg_odom_type) doubles of LDS and not one more.  The
stand-alone driver (CPU build, its own main, as in test_hostsim_sanitizers.py) therefore swaps Sim::lds for a fresh allocation of
exactly that length before the first tick — what the device gets is what ASan guards — and steps every leg count with and without
foot-position states through 3 N + 5 ticks with swinging feet; a non-finite entry of x or of the covariance fails it too.
What it can see: kf_predict carves 2 ns^2 + ns doubles and kf_correct 2 nm^2 + nm + 2 ns nm + ns^2 + ns, both from the start, so
KfScratch::len leaves 2 ns^2 + 32 doubles beyond the longer carve; with one double less than that carve ASan stops the driver at
kf_correct's store into xn.
(-DHS_KF_ONLY leaves the MHE branch of hs_update out of the build: the solve kernels' instantiation is minutes of compile time under ASan
and nothing here runs them.)"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = r'''
#include "hostsim.cpp"
#include <cmath>
#include <cstdio>
static int run(int L, int nj, int N, int ft) {
    dekf_params p; default_params(&p); p.ekf_rate = 200; p.num_legs = L; p.joints_per_leg = nj; p.N = N; p.leg_odom_type = ft; p.est_type = 1;
    const int ns = 9 + 3 * L * ft, steps = 3 * N + 5;
    int B = 2;
    Sim* h = (Sim*)hs_create(&p, B);
    if (!h) return 1;
    const size_t len = (size_t)KfScratch::len(L, ft);
    if (h->lds.size() < len) return 3;
    std::vector<double> exact(len, 0.0);   // capacity == size: the first double past it is ASan's
    h->lds.swap(exact);
    std::vector<double>().swap(exact);
    std::vector<double> t(B), acc(3 * B), gy(3 * B), pf(3 * L * B), J(3 * L * nj * B), qd(L * nj * B), c(L * B);
    std::vector<double> x(ns * B), Cm((size_t)ns * ns * B);
    int bad = 0;
    for (int T = 0; T < steps; ++T) {
        for (int b = 0; b < B; ++b) {
            t[b] = 0.005 * T + 1e-5 * b;
            acc[3*b] = 0.1; acc[3*b+1] = -0.05; acc[3*b+2] = 9.8; gy[3*b] = 0.01; gy[3*b+1] = 0.02; gy[3*b+2] = 0.2;
            for (int i = 0; i < 3 * L; ++i) pf[3*L*b + i] = 0.1 * (i % 3) - 0.25;
            for (int i = 0; i < 3 * L * nj; ++i) J[3*L*nj*b + i] = (i % (nj + 1) == 0) ? 0.2 : 0.03 * ((i + T) % 5);
            for (int i = 0; i < L * nj; ++i) qd[L*nj*b + i] = 0.1 * ((i + T) % 7) - 0.3;
            for (int i = 0; i < L; ++i) c[L*b + i] = ((T / 5 + i) % 2) ? 1.0 : 0.0;
        }
        hs_push_imu(h, t.data(), acc.data(), gy.data());
        hs_push_leg(h, pf.data(), J.data(), qd.data(), c.data());
        hs_ekf_step(h);
        if (T == 0) hs_initialize(h); else hs_update(h, T);
        hs_get(h, x.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        hs_get_kf_cov(h, Cm.data());
        for (double v : x) bad += !std::isfinite(v);
        for (double v : Cm) bad += !std::isfinite(v);
        // (variances stay positive with 9 states.  With foot states the covariance-form update takes a foot's variance from dt^2 1e14 to
        // 1e-5 at touch-down, and on THIS log — two feet with one and the same measurement coming down together — rounding leaves leg 2
        // of the 4-leg shape at -3.8e-5 for one tick where the oracle holds 5.0e-6; the make_streams logs of test_kf_mode.py keep every
        // variance positive.  The conditioning is the model's, test_foot_states.py: finite-ness only here)
        for (int b = 0; b < B && !ft; ++b)
            for (int i = 0; i < ns; ++i) bad += !(Cm[((size_t)b * ns + i) * ns + i] > 0.0);
    }
    std::printf("L=%d nj=%d N=%d leg_odom_type=%d: scratch %zu doubles, %d ticks, v=%g C_vv=%g, %d bad entries\n", L, nj, N, ft, len, steps,
                x[3], Cm[3 * ns + 3], bad);
    hs_destroy(h);
    return bad ? 2 : 0;
}
int main() {
    int rc = 0;
    for (int ft = 0; ft < 2; ++ft) rc |= run(1, 3, 5, ft) | run(2, 5, 5, ft) | run(3, 6, 5, ft) | run(4, 3, 5, ft);
    return rc;
}
'''


def test_kf_cores_are_clean_in_exactly_their_scratch(tmp_path):
    src = tmp_path / "kf_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "kf_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-DDEKF_HOSTSIM", "-DHS_KF_ONLY", "-w", "-I", os.path.join(HERE, "hostsim"),
                           "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(", 0 bad entries") == 8, r.stdout
