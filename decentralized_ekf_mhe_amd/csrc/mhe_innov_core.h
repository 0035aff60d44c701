// mhe_innov_core.h — the innovation statistics of a direct handle (dekf_set_innovation): the innovation of the newest step's leg
// measurement, its covariance, the normalised innovation squared (NIS), whole and per leg, and the predictive log-likelihood of the
// tick.  A kernel of its own behind the direct solve (kernels.hip: k_mhe_innov_*), one wavefront per instance; the direct kernels and
// mhe_direct_core.h are the code they were.
//
// What is asked for is the prediction of y_T from everything the window knows except y_T itself: x^- and P^-, the newest state and
// its covariance of the window QP with the newest step's Meas rows made free, then nu = y - H x^- and S = H P^- H' + Q_m^-1.  No
// second elimination is needed.  The direct solve ends with the POSTERIOR of the newest block, Lambda = M + H'Q H (M: what the
// window says without y_T, so P^- = M^-1), x_T = Lambda^-1 r (s.x_mhe) and P = Lambda^-1 (cov[b]), and the newest record holds y
// (Rec::BM) and Q = Q_m (Rec::qm).  With e = y - H x_T, by Woodbury on Lambda = M + H'Q H:
//     S^-1 = Q - Q H P H'Q  =: W            nu = S Q e            NIS = nu'S^-1 nu = (Q e)'S (Q e)            log det S = -log det W
// H is structural (hcol of mhe_direct_core.h with FT = 0): every leg's three rows read the velocity block with coefficient 1, so
// H P H' is P_vv = P[3:6, 3:6] in every 3 x 3 block and H x_T is the velocity in every leg block.
// Numerics: Q_m spans 1e-14 (a leg in flight) .. 1e3 and more (a stance leg) inside one matrix, so W is inverted through the
// symmetric diagonal scaling of direct_inverse (D W D, D = diag(W_ii^-1/2)), with the positive-pivot test; log det W is the sum of
// the logarithms of the scaled pivots and of W_ii.  With leg_odom_type 0, H P^- H' stays three orders below Q_m^-1 and the
// subtraction in W loses no digits.  With foot-position states it does (a foot that touches down carries a prior variance of about
// 1e14 against a measurement variance of about 1e-6: Q - Q H P H'Q cancels completely), which is why this core has no FT argument.
#pragma once
#include "cfg.h"
#include "mhe_direct_core.h"

namespace dekf {

// The stores of an innovation handle, [B][...] each: nu [nm] | S [nm][nm] | nis | nis_leg [L] | loglik: 3L + 9L^2 + 2 + L doubles
// per instance.
struct InnovStore {
    double* nu = nullptr;
    double* S = nullptr;
    double* nis = nullptr;
    double* nis_leg = nullptr;
    double* loglik = nullptr;
    DEKF_HD static size_t len(int L) { return (size_t)(3 * L + 9 * L * L + 2 + L); }
};

// LDS of one instance (doubles): Q H P (nm x 3) | g (nm) | nu (nm) | W (nm^2) | W^-1 (nm^2) | d (nm) | scratch of the lane-sequential
// inverse (2 nm)
struct InnovScratch {
    DEKF_HD static int len(int L) { const int nm = 3 * L; return 2 * nm * nm + 8 * nm; }
};

// direct_inverse (mhe_direct_core.h) with the logarithm of the determinant: Wi = W^-1 through D W D, D = diag(W_ii^-1/2), by
// Gauss-Jordan in natural pivot order with the positive-pivot test; logdet = log det W = sum log(scaled pivot) + sum log W_ii (the
// pivots of the sweep are the LDL' pivots of D W D, whose determinant is det W / prod W_ii).  A function of its own: direct_inverse
// stays the instructions it is in the direct kernels.  false (group-uniform) for a pivot that is not positive and finite.
template <int NM>
DEKF_FN bool innov_inverse(const double* W, double* Wi, double* d, double* scr, double& logdet) {
    wfor(NM, [&](int i) {
        const double v = W[NM * i + i];
        d[i] = (v > 0.0 && v < 1e300) ? 1.0 / sqrt(v) : 0.0;
    });
    bool ok = true;
    for (int i = 0; i < NM; ++i) ok = ok && d[i] > 0.0;
    if (!ok) return false;
    double ld = 0.0;
    for (int i = 0; i < NM; ++i) ld += log(W[NM * i + i]);
#if DEKF_DEVICE_BUILD
    // one column per lane in registers: direct_inverse's sweep
    (void)scr;
    const int lane = DEKF_LANE();
    const int j = lane < NM ? lane : NM - 1;
    const double dj = d[j];
    double a[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) a[i] = W[NM * i + j] * d[i] * dj;
    for (int p = 0; p < NM; ++p) {
        const double piv = readlane_f64(a[0], p);
        if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }  // wave-uniform
        ld += log(piv);
        const double dv = 1.0 / piv;
        const bool is_p = lane == p;
        const double rd = (is_p ? 1.0 : a[0]) * dv;
#pragma unroll
        for (int i = 1; i < NM; ++i) {
            const double ci = readlane_f64(a[i], p);
            a[i - 1] = fma(-ci, rd, is_p ? 0.0 : a[i]);
        }
        a[NM - 1] = rd;
    }
    if (ok && lane < NM) {
#pragma unroll
        for (int i = 0; i < NM; ++i) Wi[NM * i + lane] = a[i] * d[i] * dj;
    }
    DEKF_SYNC();
#else
    // lane-sequential: direct_inverse's sweep
    double* rowp = scr;
    double* colp = scr + NM;
    wfor(NM * NM, [&](int e) { const int i = e / NM, j = e - NM * i; Wi[e] = W[e] * d[i] * d[j]; });
    for (int p = 0; p < NM && ok; ++p) {
        const double piv = Wi[p * NM + p];
        if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }
        ld += log(piv);
        wfor(2 * NM, [&](int e) {
            if (e < NM) rowp[e] = Wi[p * NM + e];
            else colp[e - NM] = Wi[(e - NM) * NM + p];
        });
        const double dv = 1.0 / piv;
        wfor(NM * NM, [&](int e) {
            const int i = e / NM, j = e - i * NM;
            Wi[e] = i == p ? (j == p ? dv : rowp[j] * dv) : (j == p ? -colp[i] * dv : Wi[e] - colp[i] * rowp[j] * dv);
        });
    }
    if (ok) wfor(NM * NM, [&](int e) { const int i = e / NM, j = e - NM * i; Wi[e] *= d[i] * d[j]; });
#endif
    logdet = ld;
    return ok;
}

// every entry of instance b's five arrays NaN
template <int L>
DEKF_FN void innovation_nan(int b, const InnovStore& out) {
    constexpr int NM = 3 * L;
    wfor(NM * NM + NM + L + 2, [&](int e) {
        if (e < NM * NM) out.S[(size_t)NM * NM * b + e] = NAN;
        else if (e < NM * NM + NM) out.nu[(size_t)NM * b + e - NM * NM] = NAN;
        else if (e < NM * NM + NM + L) out.nis_leg[(size_t)L * b + e - NM * NM - NM] = NAN;
        else if (e == NM * NM + NM + L) out.nis[b] = NAN;
        else out.loglik[b] = NAN;
    });
}

// The innovation statistics of instance b behind its direct solve: reads s.x_mhe, s.status, cov[b] = Cov(x_T) and y | Q_m of the
// newest window record (ring slot `slot`), writes the instance's entries of `out`.  sm: InnovScratch::len(L) doubles of LDS.
// NaN in all five arrays, and false, for an instance whose solve failed (DEKF_SOLVE_NUMERIC) or whose W has a pivot that is not
// positive and finite; the status is not touched.
template <int L>
DEKF_FN bool innovation_t(const DevCfg& c, const DevState& s, int b, int slot, const double* cov, const InnovStore& out, double* sm) {
    constexpr int NM = 3 * L, NM2 = NM * NM;
    double* QP = sm;          // Q H P restricted to the velocity columns, NM x 3
    double* g = QP + 3 * NM;  // Q e
    double* nu = g + NM;
    double* W = nu + NM;
    double* Wi = W + NM2;     // S
    double* d = Wi + NM2;
    double* scr = d + NM;     // 2 NM (lane-sequential inverse)
    if (s.status[b] != DEKF_SOLVE_OK) {  // group-uniform
        innovation_nan<L>(b, out);
        return false;
    }
    const double* const x = s.x_mhe + 9 * (size_t)b;
    const double* const P = cov + 81 * (size_t)b;
    const double* const rT = s.rec + ((size_t)b * c.wcap + slot) * c.rec;
    const double* const qm = rT + Rec::qm(NM);
    // Q H P (row i of leg i / 3: Q_leg's row times P_vv) and g = Q (y - H x_T)
    wfor(4 * NM, [&](int e) {
        if (e < 3 * NM) {
            const int i = e / 3, q = e - 3 * i, leg = i / 3, a = i - 3 * leg;
            double acc = 0.0;
            for (int p = 0; p < 3; ++p) acc += symget(qm + 6 * leg, a, p, 3) * P[9 * (3 + p) + 3 + q];
            QP[e] = acc;
        } else {
            const int i = e - 3 * NM, leg = i / 3, a = i - 3 * leg;
            double acc = 0.0;
            for (int t = 0; t < 3; ++t) acc += symget(qm + 6 * leg, a, t, 3) * (rT[Rec::BM + 3 * leg + t] - x[3 + t]);
            g[i] = acc;
        }
    });
    // W = Q - Q H P H'Q from its upper triangle, mirrored: symmetric to the bit
    wfor(NM2, [&](int e) {
        const int ie = e / NM, je = e - NM * ie;
        const int i = ie < je ? ie : je, j = ie < je ? je : ie;
        const int li = i / 3, lj = j / 3, cj = j - 3 * lj;
        double sub = 0.0;
        for (int q = 0; q < 3; ++q) sub += QP[3 * i + q] * symget(qm + 6 * lj, q, cj, 3);
        W[e] = (li == lj ? symget(qm + 6 * li, i - 3 * li, cj, 3) : 0.0) - sub;
    });
    double logdet_w = 0.0;
    if (!innov_inverse<NM>(W, Wi, d, scr, logdet_w)) {  // group-uniform
        innovation_nan<L>(b, out);
        return false;
    }
    // S = W^-1 from its upper triangle, mirrored, and nu = S g on the mirrored S
    wfor(NM2 + NM, [&](int e) {
        if (e < NM2) {
            const int ie = e / NM, je = e - NM * ie;
            out.S[(size_t)NM2 * b + e] = ie < je ? Wi[NM * ie + je] : Wi[NM * je + ie];
        } else {
            const int i = e - NM2;
            double acc = 0.0;
            for (int t = 0; t < NM; ++t) acc += (i < t ? Wi[NM * i + t] : Wi[NM * t + i]) * g[t];
            nu[i] = acc;
            out.nu[(size_t)NM * b + i] = acc;
        }
    });
    // per leg: nu_l'(S_ll)^-1 nu_l by the LDL' of the 3 x 3 diagonal block (upper triangle); NaN for a pivot that is not positive
    wfor(L, [&](int leg) {
        const int o = 3 * leg;
        const double s00 = Wi[NM * o + o], s01 = Wi[NM * o + o + 1], s02 = Wi[NM * o + o + 2];
        const double s11 = Wi[NM * (o + 1) + o + 1], s12 = Wi[NM * (o + 1) + o + 2], s22 = Wi[NM * (o + 2) + o + 2];
        const double l10 = s01 / s00, l20 = s02 / s00;
        const double d1 = s11 - l10 * s01;
        const double t12 = s12 - l10 * s02;
        const double l21 = t12 / d1;
        const double d2 = s22 - l20 * s02 - l21 * t12;
        const double z0 = nu[o], z1 = nu[o + 1] - l10 * z0, z2 = nu[o + 2] - l20 * z0 - l21 * z1;
        const bool pos = s00 > 0.0 && d1 > 0.0 && d2 > 0.0 && s00 < 1e300 && d1 < 1e300 && d2 < 1e300;
        out.nis_leg[(size_t)L * b + leg] = pos ? z0 * z0 / s00 + z1 * z1 / d1 + z2 * z2 / d2 : NAN;
    });
    // NIS = g'nu and loglik = -1/2 (NIS + log det S + nm log 2 pi), log det S = -log det W
    if (DEKF_LANE() == 0) {
        double nis = 0.0;
        for (int i = 0; i < NM; ++i) nis += g[i] * nu[i];
        out.nis[b] = nis;
        out.loglik[b] = -0.5 * (nis - logdet_w + NM * 1.8378770664093453);
    }
    DEKF_SYNC();
    return true;
}

}  // namespace dekf
