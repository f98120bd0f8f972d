// gk_cgs.hpp -- interface of the CGS2 Arnoldi step (gk_set_orthogonalization GK_ORTH_CGS2;
// kernels and launchers in gk_cgs.hip, its own translation unit): classical Gram-Schmidt
// with one full reorthogonalisation on FP64 columns.  A sweep is three launches --
//   cgs_dots    slab[k][b] = workgroup b's partial of <w, V_k>, k < j, every dot on the same w
//   cgs_reduce  s[k] = sum_b slab[k][b] in a fixed order (N ranks: all-reduced afterwards)
//   cgs_axpy    w_e = ((w_e - s_1 V_1,e) - s_2 V_2,e) .. - s_j V_j,e, H(k,j) (+)= s_k
// -- with no atomics, no grid barrier and no spin wait; gk_step.hip's cgs_chain strings two
// sweeps and the closing scale together.
#pragma once
#include "gk_common.hpp"

namespace gk {

constexpr int CGS_KB_DEFAULT = 8;  // columns a dots workgroup batches (8 or 16; gk_create reads GK_CGS_KB)

// Each returns hipGetLastError() of its launch.  V: column 0 of the basis, column stride ld
// doubles (even); n: the slab's unknowns; G: workgroups along the vector (<= NPMAX).
// slab: j * G doubles, row k = column k's G partials.
GK_HIDDEN hipError_t cgs_dots(int kb, bool nt, int G, const double *w, const double *V, i64 ld, int j, i64 n,
                              double *slab, hipStream_t st);
GK_HIDDEN hipError_t cgs_reduce(const double *slab, int G, int j, double *s, hipStream_t st);
// hs[k] = (hstore ? 0 : hs[k]) + s[k] by workgroup 0; norm: pout[b] = workgroup b's partial of ||w||^2
GK_HIDDEN hipError_t cgs_axpy(bool norm, bool nt, int G, double *w, const double *V, i64 ld, int j, i64 n,
                              const double *s, double *hs, int hstore, double *pout, hipStream_t st);

}  // namespace gk
