// gk_stencil.hpp -- the operator's kernels: the Poisson-5 line march with its fused
// preconditioner epilogues (k_stencil) and the one-march A M^-1 v of cbpr2 (k_right_cbpr2).
// Included by gk_op.hip alone, which owns every launch of them.
#pragma once
#include "gk_common.hpp"

namespace gk {

// --------------------------------------------------------------------------
// Poisson-5 stencil sweep with fused preconditioner epilogues
// (src/problems/poisson.f90:33-77, src/preconds/chebyshev.f90:27-37).
//
// A workgroup owns TPB*VEC consecutive points of the fast index i and marches
// over JT grid lines j, keeping lines j-1, j, j+1 of the operand in registers:
// every operand element is read from HBM once (plus one halo line per JT),
// the W/E neighbours come from the adjacent lanes by __shfl (wave64; lanes 0
// and 63 read their outer neighbour through L1).  Missing neighbours at the
// physical boundary are zeros: x + 0 is exact, so the sum ((W+E)+S)+N is
// bit-identical to the reference's separate edge / corner statements.
// Lines -1 and nlines come from the halo buffers (RCCL halo exchange on N
// GPUs) or are zero at the physical boundary.
// --------------------------------------------------------------------------
enum {
    OP_PLAIN = 0,      // y = A x
    OP_RESID = 1,      // y = b - A x                                (gmres_mgsr.f90:314-319)
    OP_CBPR2 = 2,      // x = z: zp = z/d, y = zp + alpha*(z - A zp) (chebyshev.f90:27-37)
    OP_CHEB_FIRST = 3, // x = r: d0 = r/theta; first Chebyshev iteration
    OP_CHEB_ITER = 4,  // x = d: next Chebyshev iteration
    OP_CBPR2_ADD = 5,  // x = t: OP_CBPR2's z, y = in1 + z -- the right-preconditioned update
                       // x += M^-1 t with y = in1 = the solution (read and written at the
                       // lane's own points only); z is never stored: t and x read, x written,
                       // 24 B/unknown where OP_CBPR2 + k_add move 40
};

struct StArgs {
    const double *x;    // operand, nlines*N
    const double *hlo;  // line -1 (nullptr: physical boundary)
    const double *hhi;  // line nlines (nullptr: physical boundary)
    const double *in1;  // RESID: b ; CHEB_ITER: residual r_k ; CBPR2_ADD: the vector z is added to
    const double *in2;  // CHEB_ITER: running sum z_k
    double *y;          // main output
    double *o_res;      // CHEB: r_{k+1} (nullptr on the last iteration)
    double *o_d;        // CHEB: d_{k+1} (nullptr on the last iteration)
    const double *vdot; // ACC_DOT partner vector
    double *part;       // partial slab (ACC != NONE)
    double s1, s2, s3;  // CBPR2: d, alpha ; CHEB: theta(first)/unused, c1, c2
    int N, nlines, JT;
};

template <int VEC, int OP, int ACC>
__global__ __launch_bounds__(TPB) void k_stencil(StArgs a) {
    __shared__ double sm[WAVES];
    const int N = a.N;
    const int lane = threadIdx.x & 63;
    const i64 i0 = (i64)blockIdx.x * (TPB * VEC) + (i64)VEC * threadIdx.x;
    const bool act = i0 < N;
    const int j0 = blockIdx.y * a.JT;
    const int j1 = min(j0 + a.JT, a.nlines);
    // operand transform at load (CBPR2: /d ; CHEB_FIRST: /theta)
    constexpr bool XF = (OP == OP_CBPR2 || OP == OP_CBPR2_ADD || OP == OP_CHEB_FIRST);
    const double dv = a.s1;
    double acc = 0.0;

    auto line_ptr = [&](int jj) -> const double * {
        if (jj < 0) return a.hlo;
        if (jj >= a.nlines) return a.hhi;
        return a.x + (i64)jj * N;
    };
    auto load_line = [&](int jj, double (&raw)[VEC], double (&t)[VEC]) {
        const double *p = line_ptr(jj);
        ld_vec<VEC>(p != nullptr ? p + i0 : nullptr, act && p != nullptr, raw);
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[k] = XF ? raw[k] / dv : raw[k];
    };

    if (j0 < a.nlines) {
        // lines j-1, j, j+1 in registers and line j+2 in flight while line j is computed
        double rm[VEC], rc[VEC], rp[VEC], tm[VEC], tc[VEC], tp[VEC], rn[VEC], tn[VEC];
        load_line(j0 - 1, rm, tm);
        load_line(j0, rc, tc);
        load_line(j0 + 1, rp, tp);
#pragma unroll
        for (int k = 0; k < VEC; ++k) rn[k] = tn[k] = 0.0;
        for (int j = j0; j < j1; ++j) {
            if (j + 2 <= j1) load_line(j + 2, rn, tn);
            const i64 row = (i64)j * N;
            // W/E neighbours of the lane's first / last point
            double left = __shfl_up(tc[VEC - 1], 1, 64);  // previous lane's last point
            double right = __shfl_down(tc[0], 1, 64);      // next lane's first point
            if (lane == 0 && act) left = (i0 > 0) ? a.x[row + i0 - 1] : 0.0;
            if (lane == 63 && act) right = (i0 + VEC < N) ? a.x[row + i0 + VEC] : 0.0;
            if (XF && lane == 0) left = left / dv;
            if (XF && lane == 63) right = right / dv;
            if (i0 == 0) left = 0.0;
            if (i0 + VEC >= N) right = 0.0;
            double yv[VEC];
            double in1v[VEC], in2v[VEC];
            if (OP == OP_RESID || OP == OP_CHEB_ITER || OP == OP_CBPR2_ADD) ld_vec<VEC>(a.in1 + row + i0, act, in1v);
            if (OP == OP_CHEB_ITER) ld_vec<VEC>(a.in2 + row + i0, act, in2v);
            // the dot operand is issued with the line loads, not after the store
            double vd[VEC];
            if (ACC == ACC_DOT) ld_vec<VEC>(a.vdot + row + i0, act, vd);
            double resv[VEC], dnv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double W = (k == 0) ? left : tc[k - 1];
                const double E = (k == VEC - 1) ? right : tc[k + 1];
                const double s = ((W + E) + tp[k]) + tm[k];
                const double ax = 4.0 * tc[k] - 1.0 * s;
                if (OP == OP_PLAIN) {
                    yv[k] = ax;
                } else if (OP == OP_RESID) {
                    yv[k] = in1v[k] - ax;
                } else if (OP == OP_CBPR2) {
                    yv[k] = tc[k] + a.s2 * (rc[k] - ax);
                } else if (OP == OP_CBPR2_ADD) {  // k_add's x + z on OP_CBPR2's z
                    const double z = tc[k] + a.s2 * (rc[k] - ax);
                    yv[k] = in1v[k] + z;
                } else if (OP == OP_CHEB_FIRST) {
                    // res = r - A d0 ; d1 = c1*d0 + c2*res ; z = d0 + d1
                    const double res = rc[k] - ax;
                    const double dn = a.s2 * tc[k] + a.s3 * res;
                    resv[k] = res;
                    dnv[k] = dn;
                    yv[k] = tc[k] + dn;
                } else {  // OP_CHEB_ITER
                    const double res = in1v[k] - ax;
                    const double dn = a.s2 * tc[k] + a.s3 * res;
                    resv[k] = res;
                    dnv[k] = dn;
                    yv[k] = in2v[k] + dn;
                }
            }
            if (act) {
                st_vec<VEC>(a.y + row + i0, yv);
                if (OP == OP_CHEB_FIRST || OP == OP_CHEB_ITER) {
                    if (a.o_res != nullptr) st_vec<VEC>(a.o_res + row + i0, resv);
                    if (a.o_d != nullptr) st_vec<VEC>(a.o_d + row + i0, dnv);
                }
                if (ACC == ACC_DOT) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc = acc + yv[k] * vd[k];
                } else if (ACC == ACC_NORM) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc = acc + yv[k] * yv[k];
                }
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                rm[k] = rc[k];
                tm[k] = tc[k];
                rc[k] = rp[k];
                tc[k] = tp[k];
                rp[k] = rn[k];
                tp[k] = tn[k];
            }
        }
    }
    if (ACC != ACC_NONE) {
        const double s = block_sum(acc, sm);
        if (threadIdx.x == 0) a.part[(i64)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// --------------------------------------------------------------------------
// The right-preconditioned Arnoldi operator with cbpr2, w = A (M^-1 v), as ONE
// line march (single rank, the whole grid): z = M^-1 v is never stored.
//
// Two levels in k_stencil's register scheme.  Level 1 (z, OP_CBPR2's exact
// expressions: t = v/d, z = t + alpha*(v - A t)) runs one line ahead of level 2
// (w = A z), so level 2 finds lines j-1, j, j+1 of z in registers; level 1 keeps
// lines j, j+1, j+2 of v.  Per unknown: v and the dot partner read, w written
// (24 B) where OP_CBPR2 + OP_PLAIN move 40 B.
//
// Window seams: a lane's level-2 W/E neighbour at a wave edge is a level-1 value
// of the next window, which needs v two columns out -- lanes 0 and 63 compute the
// level-1 value of the column next to their window themselves, from the two edge
// columns ea (next to the window) and eb (one further), as k_sr_march2 does.
// Line-tile seams: z of lines j0-1 and j1 is recomputed from v of lines
// j0-2 .. j1+1.  Outside the grid z is ZERO (A z drops the neighbour), not cbpr2
// of zero-padded v; v outside the grid is zero as in k_stencil.
// Every expression, the stencil's association order and the per-workgroup dot
// order are those of k_stencil on the same grid: w, and the partial slab, are
// bit-identical to OP_CBPR2 followed by OP_PLAIN.
// --------------------------------------------------------------------------
struct RcArgs {
    const double *v;    // operand, nlines*N (nlines == N: no halo lines)
    double *w;          // output
    const double *vdot; // ACC_DOT partner vector
    double *part;       // partial slab (ACC_DOT)
    double d, alpha;    // cbpr2 coefficients (chebyshev.f90:19-25)
    int N, nlines, JT;
};

template <int VEC, int ACC>
__global__ __launch_bounds__(TPB) void k_right_cbpr2(RcArgs a) {
    __shared__ double sm[WAVES];
    const int N = a.N, nl = a.nlines;
    const int lane = threadIdx.x & 63;
    const i64 i0 = (i64)blockIdx.x * (TPB * VEC) + (i64)VEC * threadIdx.x;
    const bool act = i0 < N;
    const int j0 = blockIdx.y * a.JT;
    const int j1 = min(j0 + a.JT, nl);
    const double dv = a.d, ca = a.alpha;
    const bool e0 = lane == 0, e63 = lane == 63;
    // edge columns of the window (lane 0: to its left, lane 63: to its right), clamped
    // into the line; a clamped column is one whose value is never used (grid edge)
    i64 ea = e0 ? i0 - 1 : i0 + VEC;
    i64 eb = e0 ? i0 - 2 : i0 + VEC + 1;
    const bool edge = (e0 || e63) && act;
    const bool eb_ok = e0 ? (i0 - 2 >= 0) : (i0 + VEC + 1 < N);
    ea = ea < 0 ? 0 : (ea >= N ? N - 1 : ea);
    eb = eb < 0 ? 0 : (eb >= N ? N - 1 : eb);

    // level-0 line: v (r), t = v/d at the own points, at ea (ra, ta) and at eb (tb)
    struct L0 {
        double r[VEC], t[VEC], ra, ta, tb;
    };
    struct Raw {
        double r[VEC], ra, rb;
    };
    auto raw = [&](int jj, Raw &o) {
        const bool lv = jj >= 0 && jj < nl;
        const double *p = a.v + (i64)(lv ? jj : 0) * N;
        ld_vec<VEC>(p + (act ? i0 : 0), act && lv, o.r);
        o.ra = (edge && lv) ? p[ea] : 0.0;
        o.rb = (edge && lv && eb_ok) ? p[eb] : 0.0;
    };
    auto form = [&](const Raw &q, L0 &o) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            o.r[k] = q.r[k];
            o.t[k] = q.r[k] / dv;
        }
        o.ra = q.ra;
        o.ta = q.ra / dv;
        o.tb = q.rb / dv;
    };
    // level-1 line: z at the own points and at ea
    struct L1 {
        double z[VEC], za;
    };
    // z of line jj from v of lines jj-1 (us), jj (uc), jj+1 (un)
    auto lev1 = [&](int jj, const L0 &us, const L0 &uc, const L0 &un, L1 &o) {
        double left = __shfl_up(uc.t[VEC - 1], 1, 64);
        double right = __shfl_down(uc.t[0], 1, 64);
        left = e0 ? uc.ta : left;
        right = e63 ? uc.ta : right;
        left = i0 == 0 ? 0.0 : left;
        right = i0 + VEC >= N ? 0.0 : right;
        const bool lv = jj >= 0 && jj < nl;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const double W = (k == 0) ? left : uc.t[k - 1];
            const double E = (k == VEC - 1) ? right : uc.t[k + 1];
            const double s = ((W + E) + un.t[k]) + us.t[k];
            const double ax = 4.0 * uc.t[k] - 1.0 * s;
            const double z = uc.t[k] + ca * (uc.r[k] - ax);
            o.z[k] = (lv && act) ? z : 0.0;
        }
        // the point ea: lane 0 -> W = eb, E = own point 0; lane 63 -> W = own point VEC-1, E = eb
        const double Wa = e0 ? uc.tb : uc.t[VEC - 1];
        const double Ea = e0 ? uc.t[0] : uc.tb;
        const double sa = ((Wa + Ea) + un.ta) + us.ta;
        const double axa = 4.0 * uc.ta - 1.0 * sa;
        const double za = uc.ta + ca * (uc.ra - axa);
        o.za = lv ? za : 0.0;
    };

    double acc = 0.0;
    if (j0 < nl) {
        L0 u0, u1, u2;  // v of lines j, j+1, j+2
        L1 zm, zc;      // z of lines j-1, j
        {
            Raw q0, q1, q2, q3, q4;
            raw(j0 - 2, q0);
            raw(j0 - 1, q1);
            raw(j0, q2);
            raw(j0 + 1, q3);
            raw(j0 + 2, q4);
            L0 um2, um1;
            form(q0, um2);
            form(q1, um1);
            form(q2, u0);
            form(q3, u1);
            form(q4, u2);
            lev1(j0 - 1, um2, um1, u0, zm);
            lev1(j0, um1, u0, u1, zc);
        }
        for (int j = j0; j < j1; ++j) {
            // in flight while line j is computed: v of line j+3 (unused past the tile's
            // last line) and the dot partner of line j
            Raw qn;
            if (j + 1 < j1) {
                raw(j + 3, qn);
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) qn.r[k] = 0.0;
                qn.ra = qn.rb = 0.0;
            }
            const i64 row = (i64)j * N;
            double vd[VEC];
            if (ACC == ACC_DOT) ld_vec<VEC>(a.vdot + row + (act ? i0 : 0), act, vd);
            L1 zp;  // z of line j+1
            lev1(j + 1, u0, u1, u2, zp);
            // level 2 at line j
            double left = __shfl_up(zc.z[VEC - 1], 1, 64);
            double right = __shfl_down(zc.z[0], 1, 64);
            left = e0 ? zc.za : left;
            right = e63 ? zc.za : right;
            left = i0 == 0 ? 0.0 : left;
            right = i0 + VEC >= N ? 0.0 : right;
            double yv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double W = (k == 0) ? left : zc.z[k - 1];
                const double E = (k == VEC - 1) ? right : zc.z[k + 1];
                const double s = ((W + E) + zp.z[k]) + zm.z[k];
                yv[k] = 4.0 * zc.z[k] - 1.0 * s;
            }
            if (act) {
                st_vec<VEC>(a.w + row + i0, yv);
                if (ACC == ACC_DOT) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc = acc + yv[k] * vd[k];
                }
            }
            zm = zc;
            zc = zp;
            u0 = u1;
            u1 = u2;
            form(qn, u2);
        }
    }
    if (ACC != ACC_NONE) {
        const double s = block_sum(acc, sm);
        if (threadIdx.x == 0) a.part[(i64)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

}  // namespace gk
