// gk_stencil.hpp -- the operator's kernels: the Poisson-5 line march with its fused
// preconditioner epilogues (k_stencil) and the one-march A M^-1 v of cbpr2 (k_right_cbpr2).
// Included by gk_op.hip alone, which owns every launch of them.
#pragma once
#include "gk_march.hpp"

namespace gk {

// --------------------------------------------------------------------------
// Poisson-5 stencil sweep with fused preconditioner epilogues
// (src/problems/poisson.f90:33-77, src/preconds/chebyshev.f90:27-37).
//
// The line march of gk_march.hpp on the operand x (CBPR2, CHEB_FIRST: transformed at
// load); lanes 0 and 63 read their outer neighbour through L1 (we_load).  Lines -1
// and nlines come from the halo buffers (RCCL halo exchange on N GPUs) or are zero
// at the physical boundary.
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
    double diag;        // the operator's diagonal, fl(4 + shift) (gk_march.hpp: ax5)
    int N, nlines, JT;
};

template <int VEC, int OP, int ACC>
__global__ __launch_bounds__(TPB) void k_stencil(StArgs a) {
    __shared__ double sm[WAVES];
    const int N = a.N;
    const March m = march_init<VEC>(N, a.nlines, a.JT);
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
        ld_vec<VEC>(p != nullptr ? p + m.i0 : nullptr, m.act && p != nullptr, raw);
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[k] = XF ? raw[k] / dv : raw[k];
    };

    if (m.j0 < a.nlines) {
        // lines j-1, j, j+1 in registers and line j+2 in flight while line j is computed
        double rm[VEC], rc[VEC], rp[VEC], tm[VEC], tc[VEC], tp[VEC], rn[VEC], tn[VEC];
        load_line(m.j0 - 1, rm, tm);
        load_line(m.j0, rc, tc);
        load_line(m.j0 + 1, rp, tp);
#pragma unroll
        for (int k = 0; k < VEC; ++k) rn[k] = tn[k] = 0.0;
        for (int j = m.j0; j < m.j1; ++j) {
            if (j + 2 <= m.j1) load_line(j + 2, rn, tn);
            const i64 row = (i64)j * N;
            double left, right;
            we_load<VEC, XF>(m, N, tc, a.x, row, dv, left, right);
            double yv[VEC];
            double in1v[VEC], in2v[VEC];
            if (OP == OP_RESID || OP == OP_CHEB_ITER || OP == OP_CBPR2_ADD)
                ld_vec<VEC>(a.in1 + row + m.i0, m.act, in1v);
            if (OP == OP_CHEB_ITER) ld_vec<VEC>(a.in2 + row + m.i0, m.act, in2v);
            // the dot operand is issued with the line loads, not after the store
            double vd[VEC];
            if (ACC == ACC_DOT) ld_vec<VEC>(a.vdot + row + m.i0, m.act, vd);
            double resv[VEC], dnv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double ax = ax5_at<VEC>(a.diag, k, tc, tp, tm, left, right);
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
            if (m.act) {
                st_vec<VEC>(a.y + row + m.i0, yv);
                if (OP == OP_CHEB_FIRST || OP == OP_CHEB_ITER) {
                    if (a.o_res != nullptr) st_vec<VEC>(a.o_res + row + m.i0, resv);
                    if (a.o_d != nullptr) st_vec<VEC>(a.o_d + row + m.i0, dnv);
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
    if (ACC != ACC_NONE) put_partial(acc, sm, a.part);
}

// --------------------------------------------------------------------------
// The right-preconditioned Arnoldi operator with cbpr2, w = A (M^-1 v), as ONE
// line march (single rank, the whole grid): z = M^-1 v is never stored.
//
// A two-level march (gk_march.hpp).  Level 1 (z, OP_CBPR2's exact expressions:
// t = v/d, z = t + alpha*(v - A t)) runs one line ahead of level 2 (w = A z), so
// level 2 finds lines j-1, j, j+1 of z in registers; level 1 keeps lines j, j+1,
// j+2 of v.  Per unknown: v and the dot partner read, w written (24 B) where
// OP_CBPR2 + OP_PLAIN move 40 B.
//
// Window seams: lanes 0 and 63 compute z of the column next to their window from
// the edge columns of v (edge2_init, every lane its own columns: the grouped loads
// of the short-recurrence marches were never measured here).
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
    double diag;        // the operator's diagonal, fl(4 + shift)
    int N, nlines, JT;
};

template <int VEC, int ACC>
__global__ __launch_bounds__(TPB) void k_right_cbpr2(RcArgs a) {
    __shared__ double sm[WAVES];
    const int N = a.N, nl = a.nlines;
    const March m = march_init<VEC>(N, nl, a.JT);
    const Edge2 e = edge2_init<VEC, false>(m, N);
    const double dv = a.d, ca = a.alpha;

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
        ld_vec<VEC>(p + m.il(), m.act && lv, o.r);
        o.ra = (e.on && lv) ? p[e.ea] : 0.0;
        o.rb = (e.on && lv && e.eb_ok) ? p[e.eb] : 0.0;
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
        double left, right;
        we_select<VEC>(m, e, N, uc.t, uc.ta, left, right);
        const bool lv = jj >= 0 && jj < nl;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const double ax = ax5_at<VEC>(a.diag, k, uc.t, un.t, us.t, left, right);
            const double z = uc.t[k] + ca * (uc.r[k] - ax);
            o.z[k] = (lv && m.act) ? z : 0.0;
        }
        // the edge point ea: lane 0 -> W = eb, E = own point 0; lane 63 -> W = own point VEC-1, E = eb
        const double Wa = e.e0 ? uc.tb : uc.t[VEC - 1];
        const double Ea = e.e0 ? uc.t[0] : uc.tb;
        const double axa = ax5(a.diag, uc.ta, Wa, Ea, un.ta, us.ta);
        const double za = uc.ta + ca * (uc.ra - axa);
        o.za = lv ? za : 0.0;
    };

    double acc = 0.0;
    if (m.j0 < nl) {
        L0 u0, u1, u2;  // v of lines j, j+1, j+2
        L1 zm, zc;      // z of lines j-1, j
        {
            Raw q0, q1, q2, q3, q4;
            raw(m.j0 - 2, q0);
            raw(m.j0 - 1, q1);
            raw(m.j0, q2);
            raw(m.j0 + 1, q3);
            raw(m.j0 + 2, q4);
            L0 um2, um1;
            form(q0, um2);
            form(q1, um1);
            form(q2, u0);
            form(q3, u1);
            form(q4, u2);
            lev1(m.j0 - 1, um2, um1, u0, zm);
            lev1(m.j0, um1, u0, u1, zc);
        }
        for (int j = m.j0; j < m.j1; ++j) {
            // in flight while line j is computed: v of line j+3 (unused past the tile's
            // last line) and the dot partner of line j
            Raw qn;
            if (j + 1 < m.j1) {
                raw(j + 3, qn);
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) qn.r[k] = 0.0;
                qn.ra = qn.rb = 0.0;
            }
            const i64 row = (i64)j * N;
            double vd[VEC];
            if (ACC == ACC_DOT) ld_vec<VEC>(a.vdot + row + m.il(), m.act, vd);
            L1 zp;  // z of line j+1
            lev1(j + 1, u0, u1, u2, zp);
            // level 2 at line j
            double left, right;
            we_select<VEC>(m, e, N, zc.z, zc.za, left, right);
            double yv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) yv[k] = ax5_at<VEC>(a.diag, k, zc.z, zp.z, zm.z, left, right);
            if (m.act) {
                st_vec<VEC>(a.w + row + m.i0, yv);
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
    if (ACC != ACC_NONE) put_partial(acc, sm, a.part);
}

}  // namespace gk
