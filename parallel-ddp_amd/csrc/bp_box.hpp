// Backward pass with hard control limits lo <= u_k <= hi (pendulum, cart-pole, quadrotor; pddp_set_control_limits_problems): control-limited DDP,
// Tassa, Mansard and Todorov, ICRA 2014.
//
// The same function as bp_block() (bp.hpp) wherever no control of a knot is clamped: Qx, Qu, Qxx, Qux, Quu are formed as there (the regulariser on P's diagonal for the
// B columns), the test on the full Quu that drives the rho retry stays, and with the unconstrained step inside the knot's box the gains, the step, the cost-to-go, the
// sweep operands and the expected reduction are bp_block's expressions in bp_block's operation order -- bit for bit what k_bp writes.  Where the unconstrained step
// leaves the box, du is the minimiser of 1/2 du' Quu du - Qu' du over  ucur_k - hi <= du <= ucur_k - lo  (so that ucur_k - du is inside the limits at alpha = 1), the
// rows of K of the clamped controls are zero and the free rows are Quu_ff^-1 Qux_f.  Everything behind K and du -- P, p, A - B K, B du, dJexp -- is written in bp_block's
// form, which is the one that holds for ANY K, du:  P = Qxx + K' Quu K - K' Qux - Qux' K,  p = Qx + K' Quu du - K' Qu - Qux' du.
//
// Who computes what: n + m <= 16 for the three plants, so 16 lanes serve one (problem, block of knots), four such units per wavefront, and lane c keeps COLUMN c of
// [A B], of AB2 = [A B]' (P + rho) and of H in registers (the layout of bp_cl.hpp, here for any n, m with n + m <= 16; lanes n + m .. 15 idle along).  The other operand
// of every product is a broadcast read of the unit's LDS tile.  The box step needs no exchange at all: Quu, Qu and the box (at most 4 x 4 + 4 + 8 numbers) go through
// LDS once, every lane then holds them in registers and solves the box problem REDUNDANTLY -- an active-set walk over the clamped set with
// the LU factors of Quu_ff in registers --, so the clamped set is uniform over the unit without a vote, and state lane j < n solves for its own column of K from
// the factor it already holds: no serial loop over columns.  No barriers (wsync: LDS operations of a wave retire in order).
#pragma once

#include "bp.hpp"

namespace pddp {

template <typename P, typename T>
struct BpBoxLds {                      // one unit
    static constexpr int NX = P::NX, NU = P::NU;
    T Pm[NX * NX], pv[NX], dx[NX];
    T X[NX * 16];                      // AB2[j][column]
    T Huu[NU * NU], adj[NU * NU], Hinv[NU * NU];
    T HUX[NX * NU];                    // H[kx * NM + NX + j]  at [kx * NU + j]
    T G[16];
    T K[NX * NU];                      // bp_block's s.K[ky + NU * kx]  at [kx * NU + ky]
    T du[NU];
    T Bm[NU * NX];                     // AB[(NX + j) * NX + kx]  at [j * NX + kx]
    T box[2 * NU];                     // the knot's box for du: ucur - hi | ucur - lo
};

#define PDDP_BOX_UNROLL _Pragma("unroll")

constexpr int kBoxQpMaxIter = 32;      // faces visited per knot; a knot that needs more fails its backward pass (the rho retry)

// LU factors (no pivoting: Q is positive definite up to the regulariser's asymmetry) of Q with the rows and columns of the clamped controls (bit i of cm) replaced by
// those of the identity.  Q(i, j) = Q[j * NU + i], ALL of it: the recursion's Quu is not exactly symmetric (rho enters one of the two off-diagonal blocks of H, bp.hpp),
// the unconstrained step is Quu^-1 Qu with that matrix, and the clamped step solves Quu_ff du_f = Qu_f - Quu_fc du_c with the same one.  L: row i holds the multipliers
// left of the diagonal and U's entries from it on; Ld: the reciprocals of the pivots.  false: a pivot that is not positive.
template <typename T, int NU>
__device__ __forceinline__ bool box_factor(const T* Q, unsigned cm, T* L, T* Ld) {
    bool ok = true;
    PDDP_BOX_UNROLL for (int i = 0; i < NU; i++)
        PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) L[i * NU + j] = (((cm >> i) | (cm >> j)) & 1u) ? T(i == j ? 1 : 0) : Q[j * NU + i];
    PDDP_BOX_UNROLL for (int k = 0; k < NU; k++) {
        ok = ok && L[k * NU + k] > T(0);
        Ld[k] = T(1) / L[k * NU + k];
        PDDP_BOX_UNROLL for (int i = k + 1; i < NU; i++) {
            const T f = L[i * NU + k] * Ld[k];
            L[i * NU + k] = f;
            PDDP_BOX_UNROLL for (int j = k + 1; j < NU; j++) L[i * NU + j] -= f * L[k * NU + j];
        }
    }
    return ok;
}
// y = (L U)^-1 r
template <typename T, int NU>
__device__ __forceinline__ void box_solve(const T* L, const T* Ld, const T* r, T* y) {
    PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
        T v = r[i];
        PDDP_BOX_UNROLL for (int k = 0; k < i; k++) v -= L[i * NU + k] * y[k];
        y[i] = v;
    }
    PDDP_BOX_UNROLL for (int i = NU - 1; i >= 0; i--) {
        T v = y[i];
        PDDP_BOX_UNROLL for (int k = i + 1; k < NU; k++) v -= L[i * NU + k] * y[k];
        y[i] = v * Ld[i];
    }
}
// The minimiser x of 1/2 x' Q x - q' x over lo <= x <= hi by an active-set walk from the projection of x (the unconstrained minimiser): solve on the face of the
// clamped set; where the face's minimiser y is feasible take it and free the clamped control whose multiplier points inward most, or stop if there is none; otherwise
// go towards y up to the first bound in the way and clamp that control there.  The value never rises and a face is not visited twice, so with NU <= 4 the walk is
// short; kBoxQpMaxIter caps it.  On success: cm = the clamped controls -- on a bound with the multiplier pointing outward --, their entries of x exactly the bound,
// the free entries the solution of Q_ff x_f = q_f - Q_fc x_c, and L, Ld the factors of Q_ff (box_factor) for the gains.  Every lane of a unit runs this on the same
// numbers.  Returns 1 where the cap is hit or a pivot fails.
template <typename T, int NU>
__device__ __forceinline__ int box_qp(const T* Q, const T* q, const T* lo, const T* hi, T* x, unsigned& cm, T* L, T* Ld) {
    PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) x[i] = tmin(tmax(x[i], lo[i]), hi[i]);
    unsigned c = 0;
    PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
        T gr = -q[i];
        PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) gr += Q[j * NU + i] * x[j];
        if ((x[i] <= lo[i] && gr > T(0)) || (x[i] >= hi[i] && gr < T(0))) c |= 1u << i;
    }
    for (int it = 0; it < kBoxQpMaxIter; it++) {
        if (!box_factor<T, NU>(Q, c, L, Ld)) return 1;
        T r[NU], y[NU];
        PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
            T v = q[i];
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) v -= ((c >> j) & 1u) ? Q[j * NU + i] * x[j] : T(0);
            r[i] = ((c >> i) & 1u) ? x[i] : v;
        }
        box_solve<T, NU>(L, Ld, r, y);                               // (a clamped row of the factor is the identity's: y_c = x_c exactly)
        T t = T(1);                                                  // the largest step towards y that stays inside, and the control that stops it
        int blk = -1; bool blk_hi = false;
        PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
            if (!((c >> i) & 1u)) {
                const T d = y[i] - x[i];
                if (y[i] < lo[i]) { const T ti = x[i] <= lo[i] ? T(0) : (lo[i] - x[i]) / d; if (ti < t || blk < 0) { t = ti; blk = i; blk_hi = false; } }
                else if (y[i] > hi[i]) { const T ti = x[i] >= hi[i] ? T(0) : (hi[i] - x[i]) / d; if (ti < t || blk < 0) { t = ti; blk = i; blk_hi = true; } }
            }
        }
        if (blk >= 0) {
            PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
                if (i == blk) x[i] = blk_hi ? hi[i] : lo[i];
                else if (!((c >> i) & 1u)) x[i] = tmin(tmax(x[i] + t * (y[i] - x[i]), lo[i]), hi[i]);
            }
            c |= 1u << blk;
            continue;
        }
        // y is feasible: the clamped control whose multiplier points inward most, beyond rounding.  The multiplier is the sum of NU + 1 terms of size |q_i|, |Q_ij y_j|,
        // so its rounding error is below (NU + 1) eps times their sum `mag`: 5 x 1.2e-7 = 6e-7 in float, 5 x 2.2e-16 = 1.1e-15 in double, and y itself carries a few eps
        // of the solve -- hence 1e-6 and 1e-14 times mag, about twice and ten times that.  A multiplier inside that band is zero for all the arithmetic can tell; such a
        // control stays clamped (either choice is a minimiser there).
        // Unreachable for a positive definite Quu: the pivot failures above (every principal block of Quu is positive definite too; the full Quu has passed bp_block's
        // test by then) and the cap (the value falls strictly from face to face, and there are 3^NU <= 81 faces, of which a walk from the projected start sees a few).
        int worst = -1; T worst_v = T(0);
        PDDP_BOX_UNROLL for (int i = 0; i < NU; i++) {
            x[i] = y[i];
            T gr = -q[i], mag = tabs(q[i]);
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) { gr += Q[j * NU + i] * y[j]; mag += tabs(Q[j * NU + i] * y[j]); }
            const T inward = (y[i] <= lo[i] ? -gr : gr) - mag * (sizeof(T) == 4 ? T(1e-6) : T(1e-14));
            if (((c >> i) & 1u) && inward > worst_v) { worst_v = inward; worst = i; }
        }
        if (worst < 0) { cm = c; return 0; }
        c &= ~(1u << worst);
    }
    return 1;
}

template <typename T, int n>
__device__ __forceinline__ void box_load_col(T* v, const T* src) {      // n consecutive values; 16-byte pieces where the plant's rows allow them
    if constexpr ((n * sizeof(T)) % 16 == 0) {
        typedef T V __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int W = 16 / sizeof(T);
        PDDP_BOX_UNROLL for (int q = 0; q < n / W; q++) { const V t = reinterpret_cast<const V*>(src)[q]; PDDP_BOX_UNROLL for (int e = 0; e < W; e++) v[q * W + e] = t[e]; }
    } else {
        PDDP_BOX_UNROLL for (int e = 0; e < n; e++) v[e] = src[e];
    }
}
template <typename T, int n>
__device__ __forceinline__ void box_store_col(T* dst, const T* v) {
    if constexpr ((n * sizeof(T)) % 16 == 0) {
        typedef T V __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int W = 16 / sizeof(T);
        PDDP_BOX_UNROLL for (int q = 0; q < n / W; q++) { V t; PDDP_BOX_UNROLL for (int e = 0; e < W; e++) t[e] = v[q * W + e]; reinterpret_cast<V*>(dst)[q] = t; }
    } else {
        PDDP_BOX_UNROLL for (int e = 0; e < n; e++) dst[e] = v[e];
    }
}

// c: this lane's column (0..15; columns NX + NU .. 15 do not exist: those lanes compute on column NX + NU - 1 and store nothing).  ucur: the problem's current controls
// [N][NU]; lim: its limit row lo_0..lo_{NU-1} | hi_0..hi_{NU-1} (an unlimited problem's: -inf.. | +inf..).  Returns 1 on a failed Quu test or box step (uniform over the unit).
template <typename P, typename T>
__device__ __forceinline__ int bp_box_block(BpBoxLds<P, T>& s, int c, const Dims& dm, int blk, const BpArgs<T>& a, const T* ucur, const T* lim) {
    constexpr int NX = P::NX, NU = P::NU, NM = NX + NU;
    static_assert(NM <= 16, "column-lane backward pass: a 16-lane unit holds a column of [A B] per lane");
    static_assert(NU == 1 || NU == 4, "the Quu test of the full matrix is bp_block's: scalar, or the 4 x 4 adjugate");
    const int N = dm.N, M = dm.M, NBk = dm.NB;
    const bool act = c < NM;
    const int cc = act ? c : NM - 1;
    const bool xl = c < NX, ul = act && c >= NX;              // state column / control column
    const T rho = a.rho, rr = cc >= NX ? rho : T(0);
    int ks = NBk * (blk + 1) - 1, iterCount;
    bool lin = true;
    T dj0 = 0, dj1 = 0;                                       // lanes 0..NU-1: s.dJ[ind], s.dJ[NU + ind] of bp_block
    T lo[NU], hi[NU];
    PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) { lo[j] = lim[j]; hi[j] = lim[NU + j]; }
    if (ks == N - 1) {
        T* Pprev = a.Pm + NX * NX * (ks - 1); T* pprev = a.pv + NX * (ks - 1);
        const T* Hf = a.H + NM * NM * ks; const T* gf = a.g + NM * ks;
        for (int e = c; e < NX * NX; e += 16) { const T v = Hf[(e % NX) + NM * (e / NX)]; s.Pm[e] = v; Pprev[e] = v; }
        if (xl) { const T v = gf[c]; s.pv[c] = v; pprev[c] = v; }
        ks--; iterCount = NBk - 2; lin = false;
    } else {
        iterCount = NBk - 1;
        const T* bP = a.Pp + NX * NX * ks;
        for (int e = c; e < NX * NX; e += 16) s.Pm[e] = bP[e];
        if (xl) s.dx[c] = a.xcur[NX * (ks + 1) + c] - a.xprev2[NX * (ks + 1) + c];
    }
    wsync();
    if (lin) {
        const T* bp = a.pp + NX * ks;
        T v = 0;
        if (xl) { T dot = 0; for (int j = 0; j < NX; j++) dot += s.Pm[c + NX * j] * s.dx[j]; v = dot + bp[c]; }
        wsync();
        if (xl) s.pv[c] = v;
        wsync();
    }
    for (int iter = iterCount; iter >= 0; iter--, ks--) {
        const T* bAB = a.AB + NX * NM * ks; const T* bH = a.H + NM * NM * ks; const T* bg = a.g + NM * ks;
        const T* bd = a.dcur + NX * ks;
        T col[NX];                                            // column cc of [A B]
        box_load_col<T, NX>(col, bAB + cc * NX);
        const T gcost = bg[cc];
        T hcost[NM];
        PDDP_BOX_UNROLL for (int ky = 0; ky < NM; ky++) hcost[ky] = bH[ky * NM + cc];
        if (ul) {                                             // the knot's box for du, from the control lanes to everybody
            const T uc = ucur[NU * ks + (c - NX)];
            s.box[c - NX] = uc - lim[NU + c - NX]; s.box[NU + c - NX] = uc - lim[c - NX];
        }
        // AB2[ky][c] = sum_j AB[c][j] (P[ky][j] + [B column and ky == j] rho)
        T ab2[NX];
        PDDP_BOX_UNROLL for (int ky = 0; ky < NX; ky++) {
            T val = 0;
            PDDP_BOX_UNROLL for (int j = 0; j < NX; j++) val += col[j] * (s.Pm[ky * NX + j] + (ky == j ? rr : T(0)));
            ab2[ky] = val;
            if (ky & 1) __builtin_amdgcn_sched_barrier(0);    // (as in bp_cl.hpp: the broadcast reads stay next to their products)
        }
        const bool bnd = M > 1 && dm.on_defect_boundary(iter);        // tests the loop counter like the reference (bpHelpers.cuh:73)
        T padd = 0;
        if (bnd && xl) { T val = 0; for (int j = 0; j < NX; j++) val += bd[j] * s.Pm[c + j * NX]; padd = val; }
        PDDP_BOX_UNROLL for (int j = 0; j < NX; j++) s.X[j * 16 + c] = ab2[j];      // (an idle lane writes its own unused column)
        if (ul) { PDDP_BOX_UNROLL for (int kx = 0; kx < NX; kx++) s.Bm[(c - NX) * NX + kx] = col[kx]; }
        wsync();
        if (bnd && xl) s.pv[c] += padd;
        wsync();
        // H[ky][c] = sum_j AB2[j][ky] AB[c][j] + H_cost;   g[c] = sum_j p[j] AB[c][j] + g_cost
        T h[NM];
        PDDP_BOX_UNROLL for (int ky = 0; ky < NM; ky++) {
            T dot = 0;
            PDDP_BOX_UNROLL for (int j = 0; j < NX; j++) dot += s.X[j * 16 + ky] * col[j];
            h[ky] = dot + hcost[ky];
            if (ky & 1) __builtin_amdgcn_sched_barrier(0);
        }
        T gc;
        { T dot = 0; PDDP_BOX_UNROLL for (int j = 0; j < NX; j++) dot += s.pv[j] * col[j]; gc = dot + gcost; }
        s.G[c] = gc;
        if (ul) {
            PDDP_BOX_UNROLL for (int q = 0; q < NU; q++) s.Huu[q * NU + (c - NX)] = h[NX + q];          // H[oHUU + (e % NU) + NM (e / NU)]
            PDDP_BOX_UNROLL for (int kx = 0; kx < NX; kx++) s.HUX[kx * NU + (c - NX)] = h[kx];          // H[oHUX + kx NM + j]
        }
        wsync();
        // Quu, Qu and the box in every lane's registers from here on
        T Q[NU * NU], qu[NU], blo[NU], bhi[NU];
        PDDP_BOX_UNROLL for (int e = 0; e < NU * NU; e++) Q[e] = s.Huu[e];
        PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) { qu[j] = s.G[NX + j]; blo[j] = s.box[j]; bhi[j] = s.box[NU + j]; }
        T* bKT = a.KT + NX * NU * ks; T* bdu = a.du + NU * ks;
        T k[NU], duv[NU];                                     // lane kx < NX: K[ky][kx] = bp_block's s.K[ky + NU kx]; every lane: du
        PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) k[j] = T(0);
        // ---- the unconstrained step, bp_block's test on the full Quu included
        if constexpr (NU == 1) {                              // scalar Huu (computeKTdu_dim1)
            if (Q[0] <= T(0)) return 1;
            const T val = T(1) / Q[0];
            if (xl) k[0] = s.HUX[c] * val;
            duv[0] = qu[0] * val;
        } else {                                              // adjugate inverse with a det > 0 test (invHuu_dim4): lane e computes cofactor e
            const int ky = c / 4, kx = c % 4;
            const int r0 = (kx + 1) % 4, c0 = (ky + 1) % 4, r1 = (r0 + 1) % 4, c1 = (c0 + 1) % 4, r2 = (r1 + 1) % 4, c2 = (c1 + 1) % 4;
            const T* A2 = s.Huu;
            const T f0 = A2[c0 * 4 + r0], f1 = A2[c0 * 4 + r1], f2 = A2[c0 * 4 + r2];
            const T f3 = A2[c1 * 4 + r0], f4 = A2[c1 * 4 + r1], f5 = A2[c1 * 4 + r2];
            const T f6 = A2[c2 * 4 + r0], f7 = A2[c2 * 4 + r1], f8 = A2[c2 * 4 + r2];
            const T cdet = f0 * f4 * f8 + f3 * f7 * f2 + f6 * f1 * f5 - f2 * f4 * f6 - f5 * f7 * f0 - f8 * f1 * f3;
            const T mine = ((kx + ky) % 2 ? T(-1) : T(1)) * cdet;
            s.adj[ky * 4 + kx] = mine;
            wsync();
            const T val = T(1) / (s.adj[0] * A2[0] + s.adj[1] * A2[1] + s.adj[2] * A2[2] + s.adj[3] * A2[3]);
            if (val <= T(0)) return 1;
            s.Hinv[kx * 4 + ky] = val * mine;
            wsync();
            if (xl) {
                PDDP_BOX_UNROLL for (int r = 0; r < NU; r++) {
                    T dot = 0;
                    PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) dot += s.Hinv[r + NU * j] * s.HUX[c * NU + j];
                    k[r] = dot;
                }
            }
            PDDP_BOX_UNROLL for (int r = 0; r < NU; r++) {
                T dot = 0;
                PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) dot += s.Hinv[r + NU * j] * qu[j];
                duv[r] = dot;
            }
        }
        // ---- the box step: only where the unconstrained step leaves the box (every lane of the unit decides on the same numbers)
        bool out = false;
        PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) out = out || duv[j] < blo[j] || duv[j] > bhi[j];
        if (out) {
            unsigned cm = 0;
            T L[NU * NU], Ld[NU];
            if (box_qp<T, NU>(Q, qu, blo, bhi, duv, cm, L, Ld)) return 1;
            T r[NU];                                          // this state lane's column of K: zero rows for the clamped controls, Quu_ff^-1 Qux_f for the free ones
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) r[j] = ((cm >> j) & 1u) ? T(0) : s.HUX[cc < NX ? cc * NU + j : j];
            box_solve<T, NU>(L, Ld, r, k);
            if (!xl) { PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) k[j] = T(0); }
        }
        if (xl) { PDDP_BOX_UNROLL for (int r = 0; r < NU; r++) { s.K[c * NU + r] = k[r]; bKT[c + NX * r] = k[r]; } }
        if (c < NU) { s.du[c] = duv[c]; bdu[c] = duv[c]; }
        wsync();
        const bool do_ctg = (iter != 0 || blk != 0);
        T w[NU];                                              // lane kx < NX: (K' Huu - Hxu)[kx][ky] = bp_block's AB2[ky NX + kx]
        PDDP_BOX_UNROLL for (int ky = 0; ky < NU; ky++) {
            T val = 0;
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) val += k[j] * Q[ky * NU + j];
            w[ky] = val - h[NX + ky];
        }
        if (M > 1 && xl) {                                    // forward-sweep operands: lane ky writes column ky of A - B K, lane kx entry kx of B du
            T* bApBK = a.ApBK + NX * NX * ks; T* bBdu = a.Bdu + NX * ks;
            T outc[NX];
            PDDP_BOX_UNROLL for (int kx = 0; kx < NX; kx++) {
                T val = 0;
                PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) val += s.Bm[j * NX + kx] * k[j];
                outc[kx] = col[kx] - val;
            }
            box_store_col<T, NX>(bApBK + c * NX, outc);
            T val = 0;
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) val += s.Bm[j * NX + c] * duv[j];
            bBdu[c] = val;
        }
        if (c < NU) {                                         // expected reduction, per-lane partial sums (computeExpRed)
            T dot = 0;
            PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) dot += Q[j * NU + c] * duv[j];
            dj0 += duv[c] * qu[c];
            dj1 += duv[c] * dot;
        }
        if (do_ctg) {
            T* Pprev = a.Pm + NX * NX * (ks - 1); T* pprev = a.pv + NX * (ks - 1);
            T pn[NX]; T pvn = 0;
            if (xl) {
                PDDP_BOX_UNROLL for (int ky = 0; ky < NX; ky++) {
                    T val = 0;
                    PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) val += w[j] * s.K[ky * NU + j] - k[j] * s.HUX[ky * NU + j];
                    pn[ky] = h[ky] + val;
                    if ((ky & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
                T val = 0;
                PDDP_BOX_UNROLL for (int j = 0; j < NU; j++) val += duv[j] * w[j] - k[j] * qu[j];
                pvn = gc + val;
            }
            wsync();                                          // every lane is done with the old P, p
            if (xl) {
                PDDP_BOX_UNROLL for (int ky = 0; ky < NX; ky++) { s.Pm[ky * NX + c] = pn[ky]; Pprev[ky * NX + c] = pn[ky]; }
                s.pv[c] = pvn; pprev[c] = pvn;
            }
        }
        wsync();
    }
    s.G[c] = dj0; s.X[c] = dj1;                               // dJexp of the block = the sum of the per-lane partials in lane order (bp_block): lanes 1..NU-1 hand theirs over
    wsync();
    if (c == 0) {
        T a0 = s.G[0], a1 = s.X[0];
        for (int j = 1; j < NU; j++) { a0 += s.G[j]; a1 += s.X[j]; }
        a.dJexp[2 * blk] = a0; a.dJexp[2 * blk + 1] = a1; a.err[blk] = 0;
    }
    return 0;
}

}  // namespace pddp
