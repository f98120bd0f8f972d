// gk_step_kernels.hpp -- CDNA4 (gfx950) HIP kernels for the GMRES(m) inner cycle: the
// streaming kernels every Arnoldi path launches.  Included by gk_step.hip only.
//
// Every kernel is HBM-bandwidth bound (fp64, ~0.1-0.3 flop/B), so the design
// rules are: 16-byte (double2) coalesced accesses along the fast grid index i,
// enough independent loads in flight per wave, one pass over each vector per
// launch, and reductions that never leave the device.  No MFMA: nothing here
// is GEMM-shaped except the off-metric Gram diagnostic.
//
// Reductions are deterministic: every producer writes one partial per
// workgroup into a fixed-length slab; the consumer kernel (the next launch in
// the MGS chain) re-reduces the slab in a fixed order in its prologue
// ("launch-boundary reduce", cdna_hip_programming.md 5, item 2), so a dot
// product never needs an atomic, a grid barrier or a host round trip, and on
// N GPUs the slab itself is what RCCL all-reduces.
//
// Compiled with -ffp-contract=off: elementwise results are bit-identical to
// the CPU oracle (same association order as the Fortran reference); only the
// dot-product summation order differs.
#pragma once
#include "gk_common.hpp"

namespace gk {

// --------------------------------------------------------------------------
// Projection kernel: the MGS-R / Householder inner cascade
// (gmres_mgsr.f90:343-358, gmres_hh.f90:269-304).
//
//   h    = sum(pin[0..npin))            (the previous launch's dot, reduced)
//   w   -= (coef*h) * va                (AXPY with the just-finished dot)
//   acc += w * vb   or   w * w          (the NEXT dot, fused into the same pass)
//
// One launch = one AXPY of projection i fused with the dot of projection i+1:
// reads w, va, vb and writes w (32 B/unknown) where the reference's separate
// dot + AXPY move 40 B/unknown.
//
// T = float: va / vb are columns of the FP32-stored basis (gk_cb.hpp), widened exactly
// on load -- 24 B/unknown; w, h, the dot and every expression stay FP64.  Only
// PJ_AXPY_DOT / PJ_AXPY_NORM are instantiated, and `coef` / `blocked` / `tail0` are compiled
// out (the MGS-R chain is all float columns ever had: coef 1, grid-stride, no tail0).
// MODE: PJ_* (gk_common.hpp).
// --------------------------------------------------------------------------
template <int MODE, bool NT = false, int U = UNR, class T = double>
__global__ __launch_bounds__(TPB) void k_proj(double *__restrict__ w, const T *__restrict__ va,
                                              const T *__restrict__ vb,
                                              const double *__restrict__ pin, int npin,
                                              double *__restrict__ pout, double *__restrict__ hslot,
                                              double coef, i64 n, i64 tail0, int blocked,
                                              int hstore) {
    __shared__ double sm[WAVES];
    const i64 n2 = n >> 1;
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(w);
    typedef Col<T> C;
    constexpr bool F64 = std::is_same<T, double>::value;
    static_assert(F64 || MODE == PJ_AXPY_DOT || MODE == PJ_AXPY_NORM, "float columns: the MGS-R chain's two forms");
    const typename C::m2 *__restrict__ A2 = reinterpret_cast<const typename C::m2 *>(va);
    const typename C::m2 *__restrict__ B2 = reinterpret_cast<const typename C::m2 *>(vb);
    // Work mapping: grid-stride over U*TPB double2 chunks; `blocked` (one contiguous
    // range per workgroup) is always 0 since GK_TUNE_PROJ_BLOCKED was retired.  The
    // argument and its branch stay for now: the kernel without them ran the
    // launch-per-projection path 3 % slower at 4096^2 (138.9-139.4 vs 143.0-144.6 it/s,
    // three interleaved pairs), so this is still the machine code that was tuned.
    i64 lo, hi, step;
    if (F64 && blocked) {
        const i64 chunk = (i64)TPB * U;
        const i64 per = ((n2 + gridDim.x - 1) / gridDim.x + chunk - 1) / chunk * chunk;
        lo = (i64)blockIdx.x * per;
        hi = min(lo + per, n2);
        step = chunk;
    } else {
        lo = (i64)blockIdx.x * TPB * U;
        hi = n2;
        step = (i64)gridDim.x * TPB * U;
    }
    double2 wv[U];
    typename C::v2 av[U], bv[U];
    i64 idx[U];
    auto issue = [&](i64 base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 e = base + (i64)u * TPB;
            idx[u] = (e < hi) ? e : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 e = idx[u];
            if (e >= 0) {
                wv[u] = W2[e];
                if (MODE != PJ_DOT) av[u] = C::template ld<NT>(A2 + e);
                if (MODE == PJ_DOT || MODE == PJ_AXPY_DOT) bv[u] = C::template ld<NT>(B2 + e);
            }
        }
    };
    // The first chunk's loads do not depend on h: issue them before the
    // slab-reduce prologue so their latency hides behind it (matters when a
    // launch is only a few microseconds: small grids, many GPUs).
    i64 base = lo + threadIdx.x;
    if (base < hi) issue(base);
    double ch = 0.0;
    if (MODE != PJ_DOT) {
        const double h = reduce_slab(pin, npin, sm);
        // H(i,j) = H(i,j) + h: the first MGS pass starts from H(i,j) = 0
        if (hslot != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *hslot = (hstore ? 0.0 : *hslot) + h;
        ch = F64 ? coef * h : h;
    }
    double acc = 0.0;
    while (base < hi) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 e = idx[u];
            if (e >= 0) {
                C::landed(av[u], bv[u]);
                if (MODE != PJ_DOT) {
                    wv[u].x = wv[u].x - ch * (double)av[u].x;
                    wv[u].y = wv[u].y - ch * (double)av[u].y;
                    W2[e] = wv[u];
                }
                if (MODE == PJ_DOT || MODE == PJ_AXPY_DOT) {
                    acc = acc + wv[u].x * (double)bv[u].x;
                    acc = acc + wv[u].y * (double)bv[u].y;
                }
                if (MODE == PJ_AXPY_NORM) {
                    if (!F64 || 2 * e >= tail0) acc = acc + wv[u].x * wv[u].x;
                    if (!F64 || 2 * e + 1 >= tail0) acc = acc + wv[u].y * wv[u].y;
                }
            }
        }
        base += step;
        if (base < hi) issue(base);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd-length tail element
        const i64 e = n - 1;
        double x = w[e];
        if (MODE != PJ_DOT) {
            x = x - ch * (double)va[e];
            w[e] = x;
        }
        if (MODE == PJ_DOT || MODE == PJ_AXPY_DOT) acc = acc + x * (double)vb[e];
        if (MODE == PJ_AXPY_NORM && (!F64 || e >= tail0)) acc = acc + x * x;
    }
    if (MODE != PJ_AXPY) {
        const double s = block_sum(acc, sm);
        if (threadIdx.x == 0) pout[blockIdx.x] = s;
    }
}

// out = w / h, h = sqrt(sum(pin)) (norm2 + scale, gmres_mgsr.f90:362-363,384).
// hslot (optional) receives h.  h == 0 (exact breakdown) writes zeros instead
// of the reference's Inf/NaN.
// hcopy (optional): block 0 also publishes hsrc[0..ncopy) and h to hcopy
// (mapped pinned host memory: the step's Hessenberg column, no extra copy).
// pin_norm: pin[0] is h itself (a norm taken in the reference's order, k_norm2_seq).
__global__ __launch_bounds__(TPB) void k_scale(double *__restrict__ out, const double *__restrict__ w,
                                               const double *__restrict__ pin, int npin,
                                               double *__restrict__ hslot, i64 n,
                                               double *__restrict__ hcopy = nullptr,
                                               const double *__restrict__ hsrc = nullptr, int ncopy = 0,
                                               int pin_norm = 0) {
    __shared__ double sm[WAVES];
    const double h = pin_norm ? pin[0] : sqrt(reduce_slab(pin, npin, sm));
    if (hslot != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *hslot = h;
    if (hcopy != nullptr && blockIdx.x == 0) {
        for (int k = threadIdx.x; k < ncopy; k += TPB) hcopy[k] = hsrc[k];
        if (threadIdx.x == 0) hcopy[ncopy] = h;
    }
    const i64 n2 = n >> 1;
    const double2 *__restrict__ W2 = reinterpret_cast<const double2 *>(w);
    double2 *__restrict__ O2 = reinterpret_cast<double2 *>(out);
    const i64 stride = (i64)gridDim.x * TPB;
    if (h != 0.0) {
        for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
            double2 v = W2[e];
            v.x = v.x / h;
            v.y = v.y / h;
            O2[e] = v;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = w[n - 1] / h;
    } else {
        for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) O2[e] = double2{0.0, 0.0};
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = 0.0;
    }
}

// out[0] = sqrt(sum(pin)) or sum(pin).
__global__ __launch_bounds__(TPB) void k_finalize(const double *__restrict__ pin, int npin,
                                                  double *__restrict__ out, int take_sqrt) {
    __shared__ double sm[WAVES];
    const double s = reduce_slab(pin, npin, sm);
    if (threadIdx.x == 0) out[0] = take_sqrt ? sqrt(s) : s;
}

// x[e] += sum_k V[k*ld + e] * y[k]  (gmres_mgsr.f90:400-406: the reference's
// row-wise dot_product(V(idx,1:n_out), y) with idx on the lane, k sequential).
// ADD = false: x[e] = that sum (t = V y of the right-preconditioned update).
// T: the type the columns are stored in (float: widened exactly on load).
template <bool ADD = true, class T = double>
__global__ __launch_bounds__(TPB) void k_update_x(double *__restrict__ x, const T *__restrict__ V,
                                                  i64 ld, const double *__restrict__ y, int nout, i64 n) {
    const i64 n2 = n >> 1;
    const i64 stride = (i64)gridDim.x * TPB;
    double2 *__restrict__ X2 = reinterpret_cast<double2 *>(x);
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
        for (int k = 0; k < nout; ++k) {
            const typename Col<T>::m2 v = reinterpret_cast<const typename Col<T>::m2 *>(V + (i64)k * ld)[e];
            const double yk = y[k];
            s0 = s0 + (double)v.x * yk;
            s1 = s1 + (double)v.y * yk;
        }
        double2 xv = ADD ? X2[e] : double2{0.0, 0.0};
        xv.x = ADD ? xv.x + s0 : s0;
        xv.y = ADD ? xv.y + s1 : s1;
        X2[e] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < nout; ++k) s = s + (double)V[(i64)k * ld + n - 1] * y[k];
        x[n - 1] = ADD ? x[n - 1] + s : s;
    }
}

// x = x + w  (gmres_hh.f90:374-378)
__global__ __launch_bounds__(TPB) void k_add(double *__restrict__ x, const double *__restrict__ w, i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) x[e] = x[e] + w[e];
}

// x[e] = deterministic pseudo-random value of the GLOBAL index g0+e in [-1,1)
// (splitmix64), identical for any slab decomposition.
__global__ __launch_bounds__(TPB) void k_fill_hash(double *__restrict__ x, i64 n, i64 g0, unsigned long long seed) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) {
        unsigned long long z = (unsigned long long)(g0 + e) + seed * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        x[e] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
}

// --------------------------------------------------------------------------
// Gram matrix of columns 0..c-1 of V (the v_err diagnostics,
// gmres_mgsr.f90:414-420, gmres_hh.f90:587-591).  Off the Arnoldi metric.
// Each workgroup stages GROWS rows x c columns in LDS and accumulates the
// c(c+1)/2 pairs it owns; slab[blk*npairs + p]; then k_gram_reduce sums the
// slab over workgroups in a fixed order.  T: the type the columns are stored in.
// --------------------------------------------------------------------------
constexpr int GROWS = 32;
constexpr int GPPT = (GCMAX * (GCMAX + 1) / 2 + TPB - 1) / TPB;  // pairs per thread

template <class T = double>
__global__ __launch_bounds__(TPB) void k_gram(const T *__restrict__ V, i64 ld, int c, i64 n,
                                              const short2 *__restrict__ pairs, int npairs,
                                              double *__restrict__ slab) {
    __shared__ double tile[GROWS][GCMAX + 1];
    double acc[GPPT];
#pragma unroll
    for (int q = 0; q < GPPT; ++q) acc[q] = 0.0;
    const i64 nchunks = (n + GROWS - 1) / GROWS;
    for (i64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const i64 r0 = ch * GROWS;
        for (int t = threadIdx.x; t < GROWS * c; t += TPB) {
            const int col = t / GROWS, r = t % GROWS;
            const i64 e = r0 + r;
            tile[r][col] = (e < n) ? (double)V[(i64)col * ld + e] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GPPT; ++q) {
            const int p = threadIdx.x + q * TPB;
            if (p < npairs) {
                const short2 ab = pairs[p];
                double s = 0.0;
#pragma unroll 8
                for (int r = 0; r < GROWS; ++r) s = s + tile[r][ab.x] * tile[r][ab.y];
                acc[q] = acc[q] + s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < GPPT; ++q) {
        const int p = threadIdx.x + q * TPB;
        if (p < npairs) slab[(i64)blockIdx.x * npairs + p] = acc[q];
    }
}

__global__ __launch_bounds__(TPB) void k_gram_reduce(const double *__restrict__ slab, int nblk, int npairs,
                                                     double *__restrict__ out) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= npairs) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s = s + slab[(i64)b * npairs + p];
    out[p] = s;
}

// out[p] = dot_product(V(:,pairs[p].x+1), V(:,pairs[p].y+1)), one lane per pair (seq_dot, gk_common.hpp).
__global__ __launch_bounds__(64) void k_seqdot_pairs(const double *__restrict__ V, i64 ld, i64 n,
                                                     const short2 *__restrict__ pairs, int npairs,
                                                     double *__restrict__ out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npairs) return;
    const short2 ab = pairs[p];
    out[p] = seq_dot(V + (i64)ab.x * ld, V + (i64)ab.y * ld, n);
}

}  // namespace gk
