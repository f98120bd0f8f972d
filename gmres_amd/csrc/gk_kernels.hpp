// gk_kernels.hpp -- CDNA4 (gfx950) HIP kernels for the GMRES(m) inner cycle.
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
#include "gk_cheb.hpp"
#include "gk_res.hpp"

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
// --------------------------------------------------------------------------
enum { PJ_DOT = 0, PJ_AXPY = 1, PJ_AXPY_DOT = 2, PJ_AXPY_NORM = 3 };

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

// y = y + a x  (host scalar a)
__global__ __launch_bounds__(TPB) void k_axpy_host(double *__restrict__ y, double a, const double *__restrict__ x,
                                                   i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) y[e] = y[e] + a * x[e];
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

// --------------------------------------------------------------------------
// Gram matrix of columns 0..c-1 of V (the v_err diagnostics,
// gmres_mgsr.f90:414-420, gmres_hh.f90:587-591).  Off the Arnoldi metric.
// Each workgroup stages GROWS rows x c columns in LDS and accumulates the
// c(c+1)/2 pairs it owns; slab[blk*npairs + p]; then k_gram_reduce sums the
// slab over workgroups in a fixed order.  T: the type the columns are stored in.
// --------------------------------------------------------------------------
constexpr int GROWS = 32;
constexpr int GCMAX = 128;
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

// --------------------------------------------------------------------------
// Reference-order dots for the orthogonality diagnostics (gmres_mgsr.f90:414-420,
// gmres_hh.f90:568-593).  Fortran dot_product is ONE running sum
// h = h + a(k)*b(k), k = 1..n.  Both diagnostics measure rounding noise, and
// the reference's figure is dominated by that running sum's own rounding, so
// the device evaluates them the same way: one lane per dot, k in order,
// multiply then add (-ffp-contract=off) -- bit-identical to the reference's
// formula on the same basis.  n dependent adds per lane: slow by design, run
// once per solve (the tree-reduced k_gram is the fast alternative).
// --------------------------------------------------------------------------
constexpr int SQ_B = 8;  // double2 per column in flight per lane

__device__ __forceinline__ double seq_dot(const double *__restrict__ a, const double *__restrict__ b, i64 n) {
    const double2 *a2 = reinterpret_cast<const double2 *>(a), *b2 = reinterpret_cast<const double2 *>(b);
    const i64 n2 = n >> 1;
    double h = 0.0;
    i64 e = 0;
    for (; e + SQ_B <= n2; e += SQ_B) {
        double2 x[SQ_B], y[SQ_B];
#pragma unroll
        for (int u = 0; u < SQ_B; ++u) {
            x[u] = a2[e + u];
            y[u] = b2[e + u];
        }
#pragma unroll
        for (int u = 0; u < SQ_B; ++u) {
            h = h + x[u].x * y[u].x;
            h = h + x[u].y * y[u].y;
        }
    }
    for (i64 k = 2 * e; k < n; ++k) h = h + a[k] * b[k];
    return h;
}

// out[p] = dot_product(V(:,pairs[p].x+1), V(:,pairs[p].y+1)), one lane per pair.
__global__ __launch_bounds__(64) void k_seqdot_pairs(const double *__restrict__ V, i64 ld, i64 n,
                                                     const short2 *__restrict__ pairs, int npairs,
                                                     double *__restrict__ out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npairs) return;
    const short2 ab = pairs[p];
    out[p] = seq_dot(V + (i64)ab.x * ld, V + (i64)ab.y * ld, n);
}

// calculate_verr's rebuild V(:,i) = P_1..P_i e_i, level s of the reflection
// order (:581-585: for chain i, j = i, i-1, .., 1): chain i >= s applies
// reflector j = i - s.  k_hh_rebuild_dot: d[i] = dot_product(V(:,i), P(:,j));
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
