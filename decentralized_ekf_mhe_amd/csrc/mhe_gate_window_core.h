// mhe_gate_window_core.h — the window of a gating handle that smooths (dekf_set_gate_smoother): the gate's correction of the newest
// block carried down the window the smoother has just left.  Runs behind gate_t (mhe_gate_core.h) in the same wavefront, for the
// instances that gated a leg (kernels.hip: k_mhe_innov_gate_*_smooth); the gate core, the innovation core and the direct kernels are
// the code they were.
//
// The smoothing kernel (mhe_direct_core.h, SMOOTH without CROSS) has left x_k and P_k of the UNGATED window in win.x / win.cov and
// T1_k in win.t1.  Gating legs at step T takes E D E' out of the newest block's information alone; u_k, Li_k and T1_k of the older
// steps never read step T's Meas rows, and the backward recursion
//     x_k = u_k + T1_k' x_{k+1}         P_k = Li_k + T1_k' P_{k+1} T1_k
// is affine in x_{k+1} and in P_{k+1}.  The gate's posterior is P' = P + U C U' with U = P E (the velocity columns of the ungated P)
// and C = (D^-1 - P_vv)^-1 (gate_t's Km), and x' = x + dx with dx = -P' E w.  So with U_{K-1} = U and dx_{K-1} = dx, for k = K-2 .. 0:
//     U_k = T1_k' U_{k+1}      dx_k = T1_k' dx_{k+1}      x_k' = x_k + dx_k      P_k' = P_k + U_k C U_k'
// C is positive definite: every covariance widens and nothing cancels.  One 9 x 9 by 9 x 4 product and one rank-3 update of 81 entries
// per step; no second elimination.  P_k' is formed from the upper triangle of the update on top of the smoother's P_k, which is
// symmetric to the bit: so is P_k'.  The newest entries are the gate's own x' and P', the values x_mhe and cov[b] were written from.
// A failed correction (gate_t: DEKF_SOLVE_NUMERIC): NaN in all K entries of both arrays, the smoother's own convention.
#pragma once
#include "cfg.h"
#include "mhe_gate_core.h"

namespace dekf {

// LDS of one instance (doubles): the gate core's, then U and U C (2 x 27, changing roles every step) | dx (2 x 9) | T1_k (81)
struct GateWindowScratch {
    static constexpr int OWN = 2 * 27 + 2 * 9 + 81;
    DEKF_HD static int len(int L) { return GateScratch::len(L) + OWN; }
};

// The window correction of instance b, which has gated a leg, over its K window steps.  corrected: what gate_t reported.  sm:
// GateWindowScratch::len(L) doubles of LDS, of which gate_t has left the first GateScratch::len(L).  leg_odom_type 0: 9 states.
template <int L>
DEKF_FN void gate_window_t(const DevCfg& c, int b, int K, bool corrected, const DirectWindow& win, double* sm) {
    constexpr int NS = 9, NS2 = 81;
    const double* const gm = sm + InnovScratch::len(L);
    const double* const Km = gm + GateScratch::KM;
    const double* const w = gm + GateScratch::W;
    const double* const P = gm + GateScratch::P;
    const double* const Pn = gm + GateScratch::PN;
    const double* const xn = gm + GateScratch::XN;
    double* U = sm + GateScratch::len(L);  // U_{k+1}
    double* Un = U + 27;                   // U_k, then U_{k+1} C in the block U_{k+1} has left
    double* dx = Un + 27;
    double* dxn = dx + 9;
    double* Tk = dxn + 9;
    double* const xw = win.x + (size_t)b * c.N * NS;
    double* const cw = win.cov + (size_t)b * c.N * NS2;
    const double* const tw = win.t1 + (size_t)b * (c.N - 1) * NS2;
    if (!corrected) {  // group-uniform: never a stale or half-corrected trajectory
        wfor(K * (NS2 + NS), [&](int e) {
            if (e < K * NS2) cw[e] = NAN;
            else xw[e - K * NS2] = NAN;
        });
        return;
    }
    // the newest block: x' and P' as the gate wrote them; U_{K-1} = P E and dx_{K-1} = -P' E w (gate_t's own sum)
    wfor(NS2 + NS + 27 + NS, [&](int e) {
        if (e < NS2) cw[(size_t)NS2 * (K - 1) + e] = Pn[e];
        else if (e < NS2 + NS) xw[NS * (K - 1) + e - NS2] = xn[e - NS2];
        else if (e < NS2 + NS + 27) {
            const int i = (e - NS2 - NS) / 3, q = e - NS2 - NS - 3 * i;
            U[3 * i + q] = P[NS * i + 3 + q];
        } else {
            const int i = e - NS2 - NS - 27;
            double acc = 0.0;
            for (int q = 0; q < 3; ++q) acc += Pn[NS * i + 3 + q] * w[q];
            dx[i] = -acc;
        }
    });
    for (int k = K - 2; k >= 0; --k) {
        const double* const tk = tw + (size_t)NS2 * k;
        double* const ck = cw + (size_t)NS2 * k;
        wfor(NS2, [&](int e) { Tk[e] = tk[e]; });
        // U_k = T1_k' U_{k+1} and dx_k = T1_k' dx_{k+1}; x_k' = x_k + dx_k
        wfor(27 + NS, [&](int e) {
            if (e < 27) {
                const int i = e / 3, q = e - 3 * i;
                double acc = 0.0;
                for (int t = 0; t < NS; ++t) acc += Tk[NS * t + i] * U[3 * t + q];
                Un[e] = acc;
            } else {
                const int i = e - 27;
                double acc = 0.0;
                for (int t = 0; t < NS; ++t) acc += Tk[NS * t + i] * dx[t];
                dxn[i] = acc;
                xw[NS * k + i] += acc;
            }
        });
        // U_k C over U_{k+1}, which is dead
        wfor(27, [&](int e) {
            const int i = e / 3, q = e - 3 * i;
            double acc = 0.0;
            for (int p = 0; p < 3; ++p) acc += Un[3 * i + p] * gate_sym3(Km, p, q);
            U[e] = acc;
        });
        // P_k' = P_k + (U_k C) U_k', the update from its upper triangle on every lane's own entry of the symmetric P_k
        wfor(NS2, [&](int e) {
            const int ie = e / NS, je = e - NS * ie;
            const int i = ie < je ? ie : je, j = ie < je ? je : ie;
            double acc = 0.0;
            for (int q = 0; q < 3; ++q) acc += U[3 * i + q] * Un[3 * j + q];
            ck[e] += acc;
        });
        double* sw = U;
        U = Un;
        Un = sw;
        sw = dx;
        dx = dxn;
        dxn = sw;
    }
}

}  // namespace dekf
