// gk_mg.hpp -- interface of the aggregation multigrid V-cycle's own kernels (GK_PREC_MG;
// kernels and launchers in gk_mg.hip, its own translation unit).  The cycle itself is a
// composition in gk_op.hip (mg_apply): every level runs the project's stencil and Chebyshev
// sweeps on a smaller square grid, and these three streaming launches move between levels
// and close the cycle --
//   mg_restrict     rc(I,J) = ((f(2I,2J) + f(2I+1,2J)) + f(2I,2J+1)) + f(2I+1,2J+1), f stored,
//                   or f = r - A z formed on the fly in gk_march.hpp's line march (never stored)
//   mg_prolong_add  out(i,j) = z(i,j) + ec(i/2, j/2)
//   mg_add          out = a + b with the fused dot / norm partials of the launch that writes out
// -- with no atomics, no grid barrier and no spin wait.  N is the FINE grid's side (even).
#pragma once
#include "gk_common.hpp"

namespace gk {

// Levels: N_0 = N; while N_l is even and N_l / 2 >= MG_NMIN, N_{l+1} = N_l / 2.
constexpr int MG_NMIN = 8;
constexpr int MG_LMAX = 32;     // more levels than an int side can have
constexpr int MG_DEG_MAX = 8;   // smoother degree: one temporal-blocked pass
constexpr int MG_CDEG_MAX = 64; // coarsest-level degree cap (gk_set_precond's Chebyshev bound)

// Pure host: the level sides into sides[0 .. MG_LMAX) and their count (0: N has no coarse
// level -- odd, or N / 2 < MG_NMIN), and the coarsest level's exact spectrum interval
// (lo, hi), moved by that level's shift, and sweep count.
GK_HIDDEN int mg_levels(int N, int *sides);
GK_HIDDEN int mg_coarse_degree(int NL, double shift, double *lo, double *hi);

// Each returns hipGetLastError() of its launch (hipErrorInvalidValue for an odd N).
// fused: rc = P^T (r - A z), x = z, r = r, A's diagonal diag = fl(4 + shift_l); else rc = P^T x
// (r, diag unused).
GK_HIDDEN hipError_t mg_restrict(bool fused, int N, double diag, const double *x, const double *r, double *rc,
                                 hipStream_t st);
GK_HIDDEN hipError_t mg_prolong_add(int N, const double *z, const double *ec, double *out, hipStream_t st);
// G workgroups (<= NPMAX); acc != ACC_NONE: part[b] = workgroup b's partial of <out, vdot> / <out, out>
GK_HIDDEN hipError_t mg_add(int acc, int G, i64 n, const double *a, const double *b, double *out, const double *vdot,
                            double *part, hipStream_t st);

}  // namespace gk
