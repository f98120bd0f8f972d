// gk_kernels.hpp -- the small vector kernels of gk_api.hip (Lanczos, the gk_vec_* primitives,
// the all-ones right-hand side).  gk_step_kernels.hpp's rules hold.  Included by gk_api.hip only.
#pragma once
#include "gk_common.hpp"

namespace gk {

// y = y + a x  (host scalar a)
__global__ __launch_bounds__(TPB) void k_axpy_host(double *__restrict__ y, double a, const double *__restrict__ x,
                                                   i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) y[e] = y[e] + a * x[e];
}

// Linear combinations of the short-recurrence solvers, in the reference's
// expression order (src/cg.f90:205-231, src/bicgstab.f90:131-180).
enum { LC_COPY = 0, LC_AXPY = 1, LC_AXPY2 = 2, LC_XPAYMZ = 3, LC_ZERO = 4 };
__global__ __launch_bounds__(TPB) void k_lincomb(int form, double *out, const double *a, const double *b,
                                                 const double *c, double s1, double s2, i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        double v;
        switch (form) {
            case LC_COPY: v = a[e]; break;
            case LC_AXPY: v = a[e] + s1 * b[e]; break;                  // a + s1 b
            case LC_AXPY2: v = a[e] + s1 * b[e] + s2 * c[e]; break;      // (a + s1 b) + s2 c
            case LC_XPAYMZ: v = a[e] + s1 * (b[e] - s2 * c[e]); break;   // a + s1 (b - s2 c)
            default: v = 0.0; break;
        }
        out[e] = v;
    }
}

__global__ __launch_bounds__(TPB) void k_fill(double *__restrict__ x, double v, i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) x[e] = v;
}

}  // namespace gk
