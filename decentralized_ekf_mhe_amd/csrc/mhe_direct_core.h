// mhe_direct_core.h — the direct MHE solve (dekf_set_solver(h, DEKF_SOLVER_DIRECT)): the exact optimum of the window QP and the
// covariance of its newest state by one forward block elimination, one wavefront per instance.
//
// The window QP (mhe_solve_core.h) has two kinds of rows only: equalities (every Meas and Dyn row, and a VO row once vision has
// written its bound) and free rows (the +-1e30 VO placeholders).  Every slack sits in exactly one row with coefficient -1 and has a
// quadratic cost of its own, so on an equality row the states fix it (s = A_x x - b, cost 1/2 (A_x x - b)' Q (A_x x - b)) and on a
// free row its optimum is 0.  What is left is an unconstrained least-squares problem in x_0 .. x_{K-1} whose information matrix is
// block tridiagonal.  Eliminating the blocks front to back carries an information pair (M, h) — cost 1/2 x'Mx - h'x on the block —
// from the arrival cost (M_p, -n_p) through the window:
//     Lambda_k = M_k + H'Q_m H [+ A'Q_d A + E'Q_c E]          r_k = h_k + H'Q_m y [+ A'Q_d b_d + E'Q_c b_c]
//     G_k = Q_d A [+ E'Q_c E]                                  Qb_k = Q_d b_d [+ E'Q_c b_c]
//     M_{k+1} = Q_d [+ E'Q_c E] - G_k Lambda_k^-1 G_k'         h_{k+1} = G_k Lambda_k^-1 r_k - Qb_k
// (H = A_meas, A = A_dyn of step k, E = [I 0] the position rows, the bracketed VO terms only when step k's VO row is an equality;
// the same algebra as marginalize_info, mhe_assemble_core.h).  The newest block has no Dyn / VO row: x_T = Lambda_{K-1}^-1 r_{K-1}
// and Cov(x_T) = Lambda_{K-1}^-1 = [J^-1]_TT.  No back-substitution: x_mhe is x_T alone.  Without VO rows this is the Kalman filter
// on the window, in information form.
//
// The window smoother (SMOOTH, dekf_set_smoother): eliminating x_k left the conditional x_k | x_{k+1} ~ N(Li_k (r_k + G_k'x_{k+1}), Li_k)
// with Li_k = Lambda_k^-1, so with u_k = Li_k r_k and T1_k = G_k Li_k (the smoother gain is T1_k') the backward (Rauch-Tung-Striebel)
// recursion gives every state of the window and its covariance:
//     x_{K-1} = u_{K-1}                 P_{K-1} = Li_{K-1}                       (what the forward pass ends with)
//     x_k = u_k + T1_k' x_{k+1}         P_k = Li_k + T1_k' P_{k+1} T1_k          k = K-2 .. 0
// G_k carries the E'Q_c E term of an equality VO row, so nothing about VO is special here.  The forward pass keeps u_k, Li_k and T1_k in
// three per-instance stores (DirectWindow, indexed by window position k, not ring slot); the backward pass, in the same kernel, turns
// the first two into x_k and P_k in place, x_{k+1} and P_{k+1} staying in LDS.  The forward pass and everything it writes are the same
// instructions on the same values with and without SMOOTH.
//
// The window cross-covariances (CROSS, dekf_set_window_cross; SMOOTH only): x_k = u_k + T1_k' x_{k+1} + e_k with e_k independent of every
// later state, so
//     W_k = Cov(x_k, x_{k+1}) = T1_k' P_{k+1}                                    (lag-one: the W of the P_k recursion)
//     Z_{K-1} = P_{K-1}      Z_k = Cov(x_k, x_T) = T1_k' Z_{k+1}                 (to-newest: one more product per step)
// W_k goes back over T1_k in its store (t1[k] is dead once step k has loaded it), Z_k into a store of its own (DirectCross).  The P_k
// recursion keeps its operations and their order: everything SMOOTH writes has the same bits with and without CROSS.
//
// Inputs are exactly what solve_window_t reads: the window records at ring slot (kstart + k) % wcap (Meas from Rec::BM / qm, Dyn
// from Rec::AS / QD and the bias gains, VO gains from Rec::QC) and, from the solve's input snapshot (DevState::snap), the arrival
// cost and the VO flag / bound of every slot.  Qd | Qc of the newest record are never read (k_mhe_marginalize_early of the next step
// may be writing them).
// Numerics: the weights span 1e-14 .. 4.4e9, so every pivot block is scaled symmetrically by its diagonal (d_i = Lambda_ii^-1/2)
// before it is inverted, and the inverse is scaled back.
#pragma once
#include "cfg.h"
#include "mhe_assemble_core.h"
#include "smallmat.h"

namespace dekf {

// LDS of one instance (doubles): M | h | Lambda | r | G | Qb | T1 | Lambda^-1 | d | scratch of the lane-sequential inverse
struct DirectScratch {
    DEKF_HD static int len(int ns) { return 5 * ns * ns + 6 * ns + 8; }
};

// The window smoother's stores (dekf_set_smoother), [B][...] each: x [N][ns] and cov [N][ns^2] are the outputs (window position k = 0
// the oldest step), t1 [N-1][ns^2] keeps T1_k between the two passes.  N ns + (2 N - 1) ns^2 doubles per instance.
struct DirectWindow {
    double* x = nullptr;
    double* cov = nullptr;
    double* t1 = nullptr;
};

// The cross-covariance stores (dekf_set_window_cross), [B][...] each: lag-one Cov(x_k, x_{k+1}) [N-1][ns^2] is DirectWindow::t1 itself,
// which the backward pass of a CROSS instantiation overwrites in place; newest [N][ns^2] receives Cov(x_k, x_T).  N ns^2 more doubles
// per instance.
struct DirectCross {
    double* newest = nullptr;
};

// Lambda^-1 from Lambda (both NS x NS row-major in LDS), through the symmetrically scaled matrix D Lambda D with D = diag(Lambda_ii^-1/2),
// by Gauss-Jordan in natural pivot order (no search: the scaled block is definite with a unit diagonal).  A definite block has positive
// pivots only (they are its LDL' pivots), so a pivot that is not positive and finite — definiteness lost to rounding, or a non-finite
// input — fails the inverse: false (group-uniform).
template <int NS>
DEKF_FN bool direct_inverse(const double* Lam, double* Li, double* d, double* scr) {
    wfor(NS, [&](int i) {
        const double v = Lam[NS * i + i];
        d[i] = (v > 0.0 && v < 1e300) ? 1.0 / sqrt(v) : 0.0;
    });
    bool ok = true;
    for (int i = 0; i < NS; ++i) ok = ok && d[i] > 0.0;
    if (!ok) return false;
#if DEKF_DEVICE_BUILD
    // one column per lane in registers, the sweep of gj_columns (mhe_assemble_core.h) with the positive-pivot test and IEEE division
    (void)scr;
    const int lane = DEKF_LANE();
    const int j = lane < NS ? lane : NS - 1;
    const double dj = d[j];
    double a[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) a[i] = Lam[NS * i + j] * d[i] * dj;
    for (int p = 0; p < NS; ++p) {
        const double piv = readlane_f64(a[0], p);
        if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }  // wave-uniform
        const double dv = 1.0 / piv;
        const bool is_p = lane == p;
        const double rd = (is_p ? 1.0 : a[0]) * dv;  // new pivot-row entry of this column (1 / pivot in the pivot column)
#pragma unroll
        for (int i = 1; i < NS; ++i) {
            const double ci = readlane_f64(a[i], p);
            a[i - 1] = fma(-ci, rd, is_p ? 0.0 : a[i]);
        }
        a[NS - 1] = rd;
    }
    if (ok && lane < NS) {
#pragma unroll
        for (int i = 0; i < NS; ++i) Li[NS * i + lane] = a[i] * d[i] * dj;
    }
    DEKF_SYNC();
#else
    // lane-sequential: winverse_definite's sweep (smallmat.h) with the positive-pivot test
    double* rowp = scr;
    double* colp = scr + NS;
    wfor(NS * NS, [&](int e) { const int i = e / NS, j = e - NS * i; Li[e] = Lam[e] * d[i] * d[j]; });
    for (int p = 0; p < NS && ok; ++p) {
        const double piv = Li[p * NS + p];
        if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }
        wfor(2 * NS, [&](int e) {
            if (e < NS) rowp[e] = Li[p * NS + e];
            else colp[e - NS] = Li[(e - NS) * NS + p];
        });
        const double dv = 1.0 / piv;
        wfor(NS * NS, [&](int e) {
            const int i = e / NS, j = e - i * NS;
            Li[e] = i == p ? (j == p ? dv : rowp[j] * dv) : (j == p ? -colp[i] * dv : Li[e] - colp[i] * rowp[j] * dv);
        });
    }
    if (ok) wfor(NS * NS, [&](int e) { const int i = e / NS, j = e - NS * i; Li[e] *= d[i] * d[j]; });
#endif
    return ok;
}

// The direct solve of instance b over window steps kstart .. kstart + K - 1 (K >= 2): writes x_mhe, v_b, the status words and
// cov[b] = Cov(x_T) ([B][NS][NS]).  sm: DirectScratch::len(NS) doubles of LDS.  Returns false for a non-positive or non-finite
// pivot or a non-finite result (status DEKF_SOLVE_NUMERIC).
// SMOOTH: also the window smoother; win's stores receive x_k and Cov(x_k) of all K window steps, k = 0 the oldest, or NaN in all K
// entries of both when the result is false.  No more LDS than without: the backward pass lives in what the forward pass left dead.
// CROSS (with SMOOTH): also the cross-covariances; win.t1's K - 1 first entries end as Cov(x_k, x_{k+1}) and cross.newest's K first
// entries receive Cov(x_k, x_T), or NaN in all of them when the result is false.  Still no more LDS.
template <int L, int FT, bool SMOOTH = false, bool CROSS = false>
DEKF_FN bool direct_solve_t(const DevCfg& c, const DevState& s, int b, int kstart, int K, double* sm, double* cov, DirectWindow win = DirectWindow(),
                            DirectCross cross = DirectCross()) {
    static_assert(SMOOTH || !CROSS, "the cross-covariances come out of the smoother's backward pass");
    constexpr int NM = 3 * L, NS = 9 + NM * FT, NS2 = NS * NS;
    // this instance's stores (SMOOTH only): u_k then x_k | Li_k then P_k | T1_k
    double* const xw = SMOOTH ? win.x + (size_t)b * c.N * NS : nullptr;
    double* const cw = SMOOTH ? win.cov + (size_t)b * c.N * NS2 : nullptr;
    double* const tw = SMOOTH ? win.t1 + (size_t)b * (c.N - 1) * NS2 : nullptr;
    double* const zw = CROSS ? cross.newest + (size_t)b * c.N * NS2 : nullptr;  // Z_k (CROSS only)
    double* M = sm;
    double* h = M + NS2;
    double* Lam = h + NS;
    double* r = Lam + NS2;
    double* G = r + NS;
    double* Qb = G + NS2;
    double* T1 = Qb + NS;
    double* Li = T1 + NS2;
    double* d = Li + NS2;
    double* scr = d + NS;  // 2 NS + 8 (lane-sequential inverse)
    const double* sn = s.snap + (size_t)c.snap_len * b;
    const double* vo = sn + NS2 + NS;
    const double dt = c.dt;
    // the arrival cost 1/2 x'M_p x + n_p'x of the first block
    wfor(NS2 + NS, [&](int e) {
        if (e < NS2) M[e] = sn[e];
        else h[e - NS2] = -sn[e];
    });
    bool ok = true;
    const double* const rT = s.rec + ((size_t)b * c.wcap + (kstart + K - 1) % c.wcap) * c.rec;  // the newest record (the tail's v_b)
    for (int k = 0; k < K; ++k) {
        const int slot = (kstart + k) % c.wcap;
        const double* const rk = s.rec + ((size_t)b * c.wcap + slot) * c.rec;
        const double* R = rk + Rec::R;
        const bool last = k == K - 1;
        const bool veq = !last && vo[4 * slot] != 0.0;  // group-uniform: step k's VO row is an equality
        // Q_d(i, t): the process gain, block diagonal [6x6 | bias diagonal | 3x3 per foot]
        auto qdyn = [&](int i, int t) -> double {
            if (i < 6) return t < 6 ? symget(rk + Rec::QD, i, t, 6) : 0.0;
            if (i < 9) return t == i ? c.Q_bias_dt2[i - 6] : 0.0;
            const int leg = (i - 9) / 3;
            return (t >= 9 + 3 * leg && t < 12 + 3 * leg) ? symget(rk + Rec::qf(NM) + 6 * leg, i - 9 - 3 * leg, t - 9 - 3 * leg, 3) : 0.0;
        };
        auto bdyn = [&](int i) -> double { return i < 3 ? -c.hdt2 * rk[Rec::AS + i] : (i < 6 ? -dt * rk[Rec::AS + i - 3] : 0.0); };
        // column i of A_meas restricted to leg `leg`: coefficient and row inside the leg block
        auto hcol = [&](int i, int leg, int& a) -> double {
            if (FT) {
                if (i < 3) { a = i; return -1.0; }
                a = i - 9 - 3 * leg;
                return (a >= 0 && a < 3) ? 1.0 : 0.0;
            }
            a = i - 3;
            return (i >= 3 && i < 6) ? 1.0 : 0.0;
        };
        if (!last) {
            // G = Q_d A and Qb = Q_d b_d (the VO terms join after Lambda has read them)
            wfor(NS2 + NS, [&](int e) {
                if (e < NS2) {
                    const int i = e / NS, j = e - NS * i;
                    double acc = 0.0;
                    for (int t = 0; t < NS; ++t) {
                        const double qv = qdyn(i, t);
                        if (qv != 0.0) acc += qv * adyn_entry(R, dt, t, j);
                    }
                    G[e] = acc;
                } else {
                    const int i = e - NS2;
                    double acc = 0.0;
                    for (int t = 0; t < 6; ++t) acc += qdyn(i, t) * bdyn(t);
                    Qb[i] = acc;
                }
            });
        }
        wfor(NS2 + NS, [&](int e) {
            if (e < NS2) {
                const int i = e / NS, j = e - NS * i;
                double acc = M[e];
                for (int leg = 0; leg < L; ++leg) {
                    int ai, aj;
                    const double ci = hcol(i, leg, ai), cj = hcol(j, leg, aj);
                    if (ci != 0.0 && cj != 0.0) acc += ci * cj * symget(rk + Rec::qm(NM) + 6 * leg, ai, aj, 3);
                }
                if (!last) {
                    for (int t = 0; t < NS; ++t) {
                        const double at = adyn_entry(R, dt, t, i);
                        if (at != 0.0) acc += at * G[NS * t + j];
                    }
                    if (veq && i < 3 && j < 3) acc += symget(rk + Rec::QC, i, j, 3);
                }
                Lam[e] = acc;
            } else {
                const int i = e - NS2;
                double acc = h[i];
                for (int leg = 0; leg < L; ++leg) {
                    int ai;
                    const double ci = hcol(i, leg, ai);
                    if (ci != 0.0) {
                        double ry = 0.0;
                        for (int t = 0; t < 3; ++t) ry += symget(rk + Rec::qm(NM) + 6 * leg, ai, t, 3) * rk[Rec::BM + 3 * leg + t];
                        acc += ci * ry;
                    }
                }
                if (!last) {
                    for (int t = 0; t < NS; ++t) {
                        const double at = adyn_entry(R, dt, t, i);
                        if (at != 0.0) acc += at * Qb[t];
                    }
                    if (veq && i < 3)
                        for (int t = 0; t < 3; ++t) acc += symget(rk + Rec::QC, i, t, 3) * vo[4 * slot + 1 + t];
                }
                r[i] = acc;
            }
        });
        if (veq) {  // G += E'Q_c E, Qb += E'Q_c b_c
            wfor(12, [&](int e) {
                if (e < 9) G[NS * (e / 3) + e % 3] += symget(rk + Rec::QC, e / 3, e % 3, 3);
                else {
                    const int i = e - 9;
                    double acc = 0.0;
                    for (int t = 0; t < 3; ++t) acc += symget(rk + Rec::QC, i, t, 3) * vo[4 * slot + 1 + t];
                    Qb[i] += acc;
                }
            });
        }
        ok = direct_inverse<NS>(Lam, Li, d, scr);
        if (!ok || last) break;  // group-uniform
        wmatmul<false, false>(T1, NS, G, NS, Li, NS, NS, NS, NS);  // G Lambda^-1
        wfor(NS2 + NS, [&](int e) {
            if (e < NS2) {
                const int i = e / NS, j = e - NS * i;
                double acc = qdyn(i, j);
                if (veq && i < 3 && j < 3) acc += symget(rk + Rec::QC, i, j, 3);
                double sub = 0.0;
                for (int t = 0; t < NS; ++t) sub += T1[NS * i + t] * G[NS * j + t];
                M[e] = acc - sub;
                if constexpr (SMOOTH) {  // what the backward pass needs of step k
                    cw[(size_t)NS2 * k + e] = Li[e];
                    tw[(size_t)NS2 * k + e] = T1[e];
                }
            } else {
                const int i = e - NS2;
                double acc = 0.0;
                for (int t = 0; t < NS; ++t) acc += T1[NS * i + t] * r[t];
                h[i] = acc - Qb[i];
                if constexpr (SMOOTH) {  // u_k = Lambda^-1 r
                    double u = 0.0;
                    for (int t = 0; t < NS; ++t) u += Li[NS * i + t] * r[t];
                    xw[NS * k + i] = u;
                }
            }
        });
    }
    // x_T = Lambda^-1 r and Cov(x_T) = Lambda^-1 of the newest block
    double* x = T1;
    double* cb = cov + (size_t)NS2 * b;
    wfor(NS2 + NS, [&](int e) {
        if (e < NS2) cb[e] = Li[e];
        else {
            const int i = e - NS2;
            double acc = 0.0;
            for (int t = 0; t < NS; ++t) acc += Li[NS * i + t] * r[t];
            x[i] = acc;
            if constexpr (CROSS) h[i] = acc;  // (h is dead: the backward pass keeps x_T there, T1's block goes to Z)
        }
    });
    bool finite = ok;
    for (int i = 0; i < NS; ++i) finite = finite && fabs(x[i]) <= 1e300;
    // the tail of solve_window_t: x_mhe, v_b (DecentralEst.cpp:179-185) and the status words; no ADMM iterate, so no residuals
    if (DEKF_LANE() == 0) {
        const double p_opti[3] = {0.016041, 0.089061, 0.0579875};
        double wxp[3], t[3], vb[3];
        cross3(rT + Rec::GY, p_opti, wxp);
        for (int a = 0; a < 3; ++a) t[a] = x[3 + a] + wxp[a];
        mv3(rT + Rec::R, t, vb);
        for (int j = 0; j < NS; ++j) s.x_mhe[NS * (size_t)b + j] = x[j];
        for (int a = 0; a < 3; ++a) s.v_b[3 * (size_t)b + a] = vb[a];
        s.status[b] = finite ? DEKF_SOLVE_OK : DEKF_SOLVE_NUMERIC;
        s.iters[b] = 0;
        s.rho_updates[b] = 0;
        s.polish_status[b] = 0;
        s.pri_res[b] = NAN;
        s.dua_res[b] = NAN;
    }
    DEKF_SYNC();
    if constexpr (SMOOTH) {
        if (!finite) {  // group-uniform: never a stale or half-written trajectory
            wfor(K * (NS2 + NS), [&](int e) {
                if (e < K * NS2) cw[e] = NAN;
                else xw[e - K * NS2] = NAN;
            });
            if constexpr (CROSS) {
                wfor((2 * K - 1) * NS2, [&](int e) {
                    if (e < K * NS2) zw[e] = NAN;
                    else tw[e - K * NS2] = NAN;
                });
            }
            return false;
        }
        // The backward pass.  M, Lambda, G, T1 and Lambda^-1 of the forward pass are dead: P_{k+1} stays where the newest block's
        // Lambda^-1 is, x_{k+1} alternates between the two halves of T1's head (x_T is in the first), and step k's operands take the rest.
        // CROSS: x_{k+1} / x_k alternate between h and Qb instead (as dead as the rest), which leaves T1's whole block to Z_{k+1}; Z_k is
        // written where W was once P_k has been formed, and the two blocks change roles every step.
        double* P = Li;
        double* Lk = M;    // Li_k
        double* Tk = G;    // T1_k
        double* W = Lam;   // T1_k' P_{k+1} (CROSS: then Z_k)
        double* Zn = T1;   // Z_{k+1} (CROSS only)
        (void)Zn;
        double* xn = CROSS ? h : x;  // x_{k+1}
        double* xo = CROSS ? Qb : x + NS;
        wfor(NS2 + NS, [&](int e) {  // the newest block: the values x_mhe and cov were written from
            if (e < NS2) {
                cw[(size_t)NS2 * (K - 1) + e] = P[e];
                if constexpr (CROSS) {  // Z_{K-1} = P_{K-1}: x_T is in h since the tail, nothing reads T1's head any more
                    zw[(size_t)NS2 * (K - 1) + e] = P[e];
                    Zn[e] = P[e];
                }
            } else {
                xw[NS * (K - 1) + e - NS2] = xn[e - NS2];
            }
        });
        for (int k = K - 2; k >= 0; --k) {
            const double* const uk = xw + NS * k;
            double* const ck = cw + (size_t)NS2 * k;
            const double* const tk = tw + (size_t)NS2 * k;
            wfor(NS2, [&](int e) {
                Tk[e] = tk[e];
                Lk[e] = ck[e];
            });
            wfor(NS2 + NS, [&](int e) {
                if (e < NS2) {
                    const int i = e / NS, j = e - NS * i;
                    double acc = 0.0;
                    for (int t = 0; t < NS; ++t) acc += Tk[NS * t + i] * P[NS * t + j];
                    W[e] = acc;
                    if constexpr (CROSS) tw[(size_t)NS2 * k + e] = acc;  // Cov(x_k, x_{k+1}) over T1_k, which this lane loaded
                } else {
                    const int i = e - NS2;
                    double acc = uk[i];
                    for (int t = 0; t < NS; ++t) acc += Tk[NS * t + i] * xn[t];
                    xo[i] = acc;
                    xw[NS * k + i] = acc;
                }
            });
            // P_k from its upper triangle, mirrored: symmetric to the bit
            wfor(NS2, [&](int e) {
                const int ie = e / NS, je = e - NS * ie;
                const int i = ie < je ? ie : je, j = ie < je ? je : ie;
                double acc = Lk[NS * i + j];
                for (int t = 0; t < NS; ++t) acc += W[NS * i + t] * Tk[NS * t + j];
                ck[e] = acc;
                P[e] = acc;  // (this phase reads W, not P)
            });
            double* sw = xn;
            xn = xo;
            xo = sw;
            if constexpr (CROSS) {
                // Z_k = T1_k' Z_{k+1}, W's product on Z_{k+1} (t ascending), over W
                wfor(NS2, [&](int e) {
                    const int i = e / NS, j = e - NS * i;
                    double acc = 0.0;
                    for (int t = 0; t < NS; ++t) acc += Tk[NS * t + i] * Zn[NS * t + j];
                    W[e] = acc;
                    zw[(size_t)NS2 * k + e] = acc;
                });
                sw = W;
                W = Zn;
                Zn = sw;
            }
        }
    }
    return finite;
}

}  // namespace dekf
