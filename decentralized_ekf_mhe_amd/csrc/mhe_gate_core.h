// mhe_gate_core.h — the innovation gate of a direct handle (dekf_set_innovation_gate): a stance leg whose per-leg NIS of this update
// exceeds the handle's bound is taken out of the solve it has just entered.  Runs behind innovation_t (mhe_innov_core.h) in the same
// wavefront (kernels.hip: k_mhe_innov_gate_*); the innovation core is called unchanged, so the five arrays are the ungated problem's.
//
// With leg_odom_type 0 a leg's contact flag changes one thing in the window QP: the leg's 3 x 3 block of Rec::qm, which the assemble
// step writes as diag(Q_swing) for contact == 0 (mhe_assemble_core.h: leg_terms_nj).  Gating leg l at step T therefore means "leg l
// was in swing at step T":
//   1. the leg's block of the newest record becomes diag(Q_swing), word for word what the assemble step writes, so every later
//      window and the arrival cost see a swing leg;
//   2. the newest posterior is corrected for it.  Every leg's three Meas rows read the velocity block with coefficient 1 (hcol of
//      mhe_direct_core.h with FT = 0), so with E the 9 x 3 selector of the velocity block, D = sum over the gated legs of
//      dQ_l = Q_l - diag(Q_swing) and w = sum dQ_l (y_l - v), v = x_T[3:6]:
//          Lambda' = Lambda - E D E'        r' = r - E sum dQ_l y_l
//          P' = Lambda'^-1 = P + P E (D^-1 - P_vv)^-1 E'P        x' = P' r' = x - P' E w
//      (Woodbury; however many legs are gated, the correction has rank 3, because they all read the same three states).  D is a sum
//      of stance gains less 1e-14 and is inverted as it is; D^-1 - P_vv is definite exactly when Lambda' is, and P_vv stays orders
//      below Q_m^-1, so the subtraction loses no digits.  Both 3 x 3 inverses go through innov_inverse: the
//      diagonally scaled sweep with the positive-pivot test.
// A pivot that is not positive and finite, or a result that is not finite: the record edit stands, the status becomes
// DEKF_SOLVE_NUMERIC and x_mhe, v_b and the covariance block are NaN; the next step solves from the records.
#pragma once
#include "cfg.h"
#include "mhe_innov_core.h"

namespace dekf {

// The stores of a gating handle: the bound (0: off) and gated [B][L], 1 for the legs the last update gated
struct GateStore {
    double nis_leg_max = 0.0;
    int* gated = nullptr;
};

// LDS of one instance (doubles): the innovation core's, then fl (4) | D (9) | D^-1 (9) | D^-1 - P_vv (9) | its inverse (9) | w (3) |
// P E K (27) | P (81) | P' (81) | x' (9) | d (3) | scratch of the lane-sequential inverse (6).  The constants are the fields' offsets
// behind the innovation core's part: what a gated instance leaves there (Km, w, the ungated P, P' and x' of a correction that
// succeeded) is what the window correction of a smoothing gate handle reads (mhe_gate_window_core.h).
struct GateScratch {
    static constexpr int FL = 0, D = FL + 4, DI = D + 9, KN = DI + 9, KM = KN + 9, W = KM + 9, PK = W + 3, P = PK + 27, PN = P + 81,
                         XN = PN + 81, DD = XN + 9, SCR = DD + 3;
    static constexpr int OWN = SCR + 6;
    DEKF_HD static int len(int L) { return InnovScratch::len(L) + OWN; }
};

// entry (i, j) of the symmetric 3 x 3 matrix whose upper triangle is in A (row-major, 3 x 3)
DEKF_FN double gate_sym3(const double* A, int i, int j) { return i <= j ? A[3 * i + j] : A[3 * j + i]; }

// The gate of instance b behind its innovation statistics (`solved`: what innovation_t returned).  cq: the configuration that holds
// the instance's Q_swing (the handle's, or the instance's row of the parameter table).  sm: GateScratch::len(L) doubles of LDS, of
// which the innovation core has used the first InnovScratch::len(L).  Returns the number of gated legs.  corrected (may be null):
// where legs were gated, whether the correction succeeded (group-uniform); untouched where none was.
template <int L>
DEKF_FN int gate_t(const DevCfg& c, const DevCfg& cq, const DevState& s, int b, int slot, double* cov, const InnovStore& out,
                   const GateStore& gs, bool solved, double* sm, bool* corrected = nullptr) {
    constexpr int NM = 3 * L;
    double* const gm = sm + InnovScratch::len(L);
    double* fl = gm + GateScratch::FL;  // 1.0 for a gated leg
    double* D = gm + GateScratch::D;
    double* Di = gm + GateScratch::DI;
    double* Kn = gm + GateScratch::KN;   // D^-1 - P_vv
    double* Km = gm + GateScratch::KM;   // its inverse
    double* w = gm + GateScratch::W;
    double* PK = gm + GateScratch::PK;   // P E K, 9 x 3
    double* P = gm + GateScratch::P;
    double* Pn = gm + GateScratch::PN;
    double* xn = gm + GateScratch::XN;
    double* d = gm + GateScratch::DD;
    double* scr = gm + GateScratch::SCR;
    int* const gated = gs.gated + (size_t)L * b;
    // the decision, by the lane that wrote the leg's NIS (NaN compares false: a failed solve or innovation gates nothing)
    wfor(L, [&](int leg) {
        const bool on = solved && out.nis_leg[(size_t)L * b + leg] > gs.nis_leg_max;
        fl[leg] = on ? 1.0 : 0.0;
        gated[leg] = on ? 1 : 0;
    });
    int ng = 0;
    for (int leg = 0; leg < L; ++leg) ng += fl[leg] != 0.0 ? 1 : 0;
    if (ng == 0) return 0;  // group-uniform: nothing else is touched
    double* const rT = s.rec + ((size_t)b * c.wcap + slot) * c.rec;
    double* const qm = rT + Rec::qm(NM);
    double* const x = s.x_mhe + 9 * (size_t)b;
    double* const cb = cov + 81 * (size_t)b;
    // P into LDS; D = sum dQ_l (upper triangle, mirrored) and w = sum dQ_l (y_l - v) from the record as the solve read it
    wfor(81 + 9 + 3, [&](int e) {
        if (e < 81) P[e] = cb[e];
        else if (e < 90) {
            const int ie = (e - 81) / 3, je = e - 81 - 3 * ie;
            const int i = ie < je ? ie : je, j = ie < je ? je : ie;
            double acc = 0.0;
            for (int leg = 0; leg < L; ++leg)
                if (fl[leg] != 0.0) acc += symget(qm + 6 * leg, i, j, 3) - (i == j ? cq.Q_swing[i] : 0.0);
            D[e - 81] = acc;
        } else {
            const int i = e - 90;
            double acc = 0.0;
            for (int leg = 0; leg < L; ++leg)
                if (fl[leg] != 0.0)
                    for (int t = 0; t < 3; ++t)
                        acc += (symget(qm + 6 * leg, i, t, 3) - (i == t ? cq.Q_swing[i] : 0.0)) * (rT[Rec::BM + 3 * leg + t] - x[3 + t]);
            w[i] = acc;
        }
    });
    // the record edit: the packed block the assemble step writes for contact == 0
    wfor(6 * L, [&](int e) {
        const int leg = e / 6, a = e - 6 * leg;
        if (fl[leg] != 0.0) qm[e] = a == 0 ? cq.Q_swing[0] : (a == 3 ? cq.Q_swing[1] : (a == 5 ? cq.Q_swing[2] : 0.0));
    });
    double ld = 0.0;
    bool ok = innov_inverse<3>(D, Di, d, scr, ld);  // group-uniform
    if (ok) {
        // D^-1 - P_vv from the upper triangles, mirrored
        wfor(9, [&](int e) {
            const int ie = e / 3, je = e - 3 * ie;
            const int i = ie < je ? ie : je, j = ie < je ? je : ie;
            Kn[e] = Di[3 * i + j] - P[9 * (3 + i) + 3 + j];
        });
        ok = innov_inverse<3>(Kn, Km, d, scr, ld);
    }
    if (ok) {
        // P E K, then P' = P + (P E K) (E'P) from its upper triangle, mirrored: symmetric to the bit
        wfor(27, [&](int e) {
            const int i = e / 3, q = e - 3 * i;
            double acc = 0.0;
            for (int p = 0; p < 3; ++p) acc += P[9 * i + 3 + p] * gate_sym3(Km, p, q);
            PK[e] = acc;
        });
        wfor(81, [&](int e) {
            const int ie = e / 9, je = e - 9 * ie;
            const int i = ie < je ? ie : je, j = ie < je ? je : ie;
            double acc = P[9 * i + j];
            for (int q = 0; q < 3; ++q) acc += PK[3 * i + q] * P[9 * (3 + q) + j];
            Pn[e] = acc;
        });
        // x' = x - P' E w
        wfor(9, [&](int i) {
            double acc = 0.0;
            for (int q = 0; q < 3; ++q) acc += Pn[9 * i + 3 + q] * w[q];
            xn[i] = x[i] - acc;
        });
        for (int i = 0; i < 9; ++i) ok = ok && fabs(xn[i]) <= 1e300 && fabs(Pn[10 * i]) <= 1e300;
    }
    // the outputs of the solve's tail again (mhe_direct_core.h): Cov(x_T), x_mhe, v_b and, where the correction failed, the status
    wfor(81, [&](int e) { cb[e] = ok ? Pn[e] : NAN; });
    if (DEKF_LANE() == 0) {
        const double p_opti[3] = {0.016041, 0.089061, 0.0579875};
        double wxp[3], t[3], vb[3];
        cross3(rT + Rec::GY, p_opti, wxp);
        for (int a = 0; a < 3; ++a) t[a] = xn[3 + a] + wxp[a];
        mv3(rT + Rec::R, t, vb);
        for (int j = 0; j < 9; ++j) x[j] = ok ? xn[j] : NAN;
        for (int a = 0; a < 3; ++a) s.v_b[3 * (size_t)b + a] = ok ? vb[a] : NAN;
        if (!ok) s.status[b] = DEKF_SOLVE_NUMERIC;
    }
    DEKF_SYNC();
    if (corrected) *corrected = ok;
    return ng;
}

}  // namespace dekf
