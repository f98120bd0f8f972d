// gk_hh_kernels.hpp -- the Householder cycle's own small kernels (the reflection chains are
// k_proj launches or resident launches).  gk_step_kernels.hpp's rules hold.  Included by
// gk_hh.hip only.
#pragma once
#include "gk_common.hpp"

namespace gk {

// out[0] = NORM2(x(0:n)) as flang-rt computes it (Norm2Accumulator<8>: a running
// max m and a scaled sum s, result m sqrt(1 + s); the tests check it against the CPU restatement) --
// the reference's serial norm2 of gmres_hh.f90:251-253,307,315, in its order.  One
// workgroup: chunks of TPB elements staged through LDS, thread 0 folds each in order
// (GK_TUNE_HH_NORM_ORDER, single rank; ~2 us per 256 elements).
__global__ __launch_bounds__(TPB) void k_norm2_seq(const double *__restrict__ x, i64 n, double *__restrict__ out) {
    __shared__ double buf[TPB];
    double mx = 0.0, s = 0.0;
    for (i64 c0 = 0; c0 < n; c0 += TPB) {
        const i64 e = c0 + threadIdx.x;
        buf[threadIdx.x] = e < n ? x[e] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = n - c0 < TPB ? (int)(n - c0) : TPB;
            for (int k = 0; k < cnt; ++k) {
                const double a = fabs(buf[k]);
                if (mx == 0.0) {
                    mx = a;
                } else if (a > mx) {
                    const double t = mx / a;
                    const double tsq = t * t;
                    s = s * tsq;
                    s = s + tsq;
                    mx = a;
                } else {
                    const double t = a / mx;
                    s = s + t * t;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = mx * sqrt(1.0 + s);
}

// x = 0 except x[gk - g0] = vals[k] for global indices gk = k in [0, nvals)
// (v_j = e_j, gmres_hh.f90:257-265; w(1:n_out) = y, :356-357).
__global__ __launch_bounds__(TPB) void k_set_prefix(double *__restrict__ x, i64 n, i64 g0,
                                                    const double *__restrict__ vals, int first,
                                                    int nvals) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const i64 g = g0 + e;
        x[e] = (g >= first && g < first + nvals) ? vals[g - first] : 0.0;
    }
}

// x = e_g (global index g): zero everywhere, `value` at global index g.
__global__ __launch_bounds__(TPB) void k_set_unit(double *__restrict__ x, i64 n, i64 g0, i64 g, double value) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) x[e] = (g0 + e == g) ? value : 0.0;
}

// Householder reflector fix-up (gmres_hh.f90:39-41, :305-318): zero global
// indices < zero_below; at global index fix_idx add delta[0]; accumulate
// sum w^2 of the result into pout.
__global__ __launch_bounds__(TPB) void k_hh_fix(double *__restrict__ w, i64 n, i64 g0, i64 zero_below,
                                                i64 fix_idx, const double *__restrict__ delta,
                                                double *__restrict__ pout) {
    __shared__ double sm[WAVES];
    const i64 stride = (i64)gridDim.x * TPB;
    const double dl = delta[0];
    double acc = 0.0;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        const i64 g = g0 + e;
        double v = w[e];
        if (g < zero_below) {
            v = 0.0;
            w[e] = v;
        } else if (g == fix_idx) {
            v = v + dl;
            w[e] = v;
        }
        acc = acc + v * v;
    }
    const double s = block_sum(acc, sm);
    if (threadIdx.x == 0) pout[blockIdx.x] = s;
}

// Householder pivot bookkeeping, one workgroup.  hb[0..j] = w(1:j+1) broadcast
// from the owning rank; pin = sum of squares of the tail.
//  start (j == 0): beta = sqrt(sum w^2); g1 = -sign(beta,w1); delta = sign(beta,w1)
//                  -> res[0] = g1, delta[0] = sign(beta, w1)          (:250-252)
//  step  (j >= 1): tmp = sqrt(tail); H(j+1,j) = w(j+1) > 0 ? -tmp : tmp
//                  -> hcol[0..j-1] = w(1:j), hcol[j] = H(j+1,j), delta = -H (:306-316)
// pin_norm: pin[0] is the norm itself (k_norm2_seq) instead of a partial slab of squares.
__global__ void k_hh_pivot(const double *__restrict__ hb, const double *__restrict__ pin, int npin,
                           int j, double *__restrict__ hcol, double *__restrict__ delta,
                           double *__restrict__ hcopy = nullptr, int pin_norm = 0) {
    __shared__ double sm[WAVES];
    const double s = pin_norm ? pin[0] : sqrt(reduce_slab(pin, npin, sm));
    if (j == 0) {
        if (threadIdx.x == 0) {
            const double w1 = hb[0];
            const double sg = copysign(fabs(s), w1);
            hcol[0] = -sg;
            delta[0] = sg;
        }
        return;
    }
    for (int k = threadIdx.x; k < j; k += blockDim.x) {
        hcol[k] = hb[k];
        if (hcopy != nullptr) hcopy[k] = hb[k];
    }
    if (threadIdx.x == 0) {
        const double H = (hb[j] > 0.0) ? -s : s;
        hcol[j] = H;
        if (hcopy != nullptr) hcopy[j] = H;
        delta[0] = -H;
    }
}

// calculate_verr's rebuild V(:,i) = P_1..P_i e_i, level s of the reflection
// order (:581-585: for chain i, j = i, i-1, .., 1): chain i >= s applies
// reflector j = i - s.  k_hh_rebuild_dot: d[i] = dot_product(V(:,i), P(:,j)), one lane
// per chain (seq_dot, gk_common.hpp);
// k_hh_rebuild_upd: V(:,i) = V(:,i) - 2.0*P(:,j)*d[i] (blockIdx.y = j).
__global__ __launch_bounds__(64) void k_hh_rebuild_dot(const double *__restrict__ Vb, const double *__restrict__ P,
                                                       i64 ld, i64 n, int s, int n_out, double *__restrict__ d) {
    const int i = s + blockIdx.x * 64 + threadIdx.x;
    if (i >= n_out) return;
    d[i] = seq_dot(Vb + (i64)i * ld, P + (i64)(i - s) * ld, n);
}

__global__ __launch_bounds__(TPB) void k_hh_rebuild_upd(double *__restrict__ Vb, const double *__restrict__ P,
                                                        i64 ld, i64 n, int s, const double *__restrict__ d) {
    const int j = blockIdx.y, i = s + j;
    double *__restrict__ v = Vb + (i64)i * ld;
    const double *__restrict__ p = P + (i64)j * ld;
    const double dd = d[i];
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) v[e] = v[e] - 2.0 * p[e] * dd;
}

}  // namespace gk
