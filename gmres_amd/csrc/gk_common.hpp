// gk_common.hpp -- definitions shared by every translation unit (gk_api.hip: the
// context; gk_step.hip and gk_hh.hip: the Arnoldi steps; gk_comm.hip: the collectives;
// gk_resident.hip and gk_blk.hip: the resident steps; gk_sr_api.hip: the short-recurrence
// solvers; gk_cheb.hip: the Chebyshev pass).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <type_traits>

// host symbols of the gk namespace that other units call but the library does not export
#define GK_HIDDEN __attribute__((visibility("hidden")))

namespace gk {

constexpr int TPB = 256;          // threads per workgroup (4 wave64)
constexpr int WAVES = TPB / 64;
constexpr int UNR = 4;            // double2 per thread per trip in the streaming kernels
constexpr int NPMAX = 4096;       // max partials in a slab

typedef long long i64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Deterministic block sum; result returned to every thread.
__device__ __forceinline__ double block_sum(double v, double *sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wid] = v;
    __syncthreads();
    double r = sm[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) r += sm[k];
    return r;
}

// Fixed-order reduction of a partial slab (length np <= NPMAX).
__device__ __forceinline__ double reduce_slab(const double *__restrict__ p, int np, double *sm) {
    double s = 0.0;
    for (int k = threadIdx.x; k < np; k += TPB) s += p[k];
    return block_sum(s, sm);
}

typedef double d2v __attribute__((ext_vector_type(2)));

// Load policy for the Krylov-basis columns: plain, or non-temporal (`nt`) so
// the once-per-launch V stream does not displace w from the Infinity Cache.
template <bool NT>
__device__ __forceinline__ double2 ldv(const double2 *p) {
    if constexpr (NT) {
        const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p));
        return double2{t.x, t.y};
    } else {
        return *p;
    }
}

// ... and a float2 of an FP32-stored column (gk_cb.hpp), held as a 2-vector
typedef float f2v __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ f2v ldf(const float2 *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(reinterpret_cast<const f2v *>(p));
    else
        return *reinterpret_cast<const f2v *>(p);
}

// The point from which a batch slot's two loaded float2 are used.  Without it the compiler
// places the widening conversions right behind each load and waits for that load before
// it issues the next one -- a pass then pays one memory round trip per chunk (measured:
// 62.7 us per projection at 4096^2 against the FP64 kernel's 29.3); with it the batch's
// loads go out back to back and the conversions follow the (counted) wait.
__device__ __forceinline__ void landed(f2v &a, f2v &b) { asm volatile("" : "+v"(a), "+v"(b)); }

// What a launch-path kernel needs to know of the type T a Krylov column is stored in:
// the element pair in memory (m2) and in registers (v2), its load, and landed().
template <class T>
struct Col;
template <>
struct Col<double> {
    typedef double2 m2;
    typedef double2 v2;
    template <bool NT>
    static __device__ __forceinline__ v2 ld(const m2 *p) { return ldv<NT>(p); }
    static __device__ __forceinline__ void landed(v2 &, v2 &) {}
};
template <>
struct Col<float> {
    typedef float2 m2;
    typedef f2v v2;
    template <bool NT>
    static __device__ __forceinline__ v2 ld(const m2 *p) { return ldf<NT>(p); }
    static __device__ __forceinline__ void landed(v2 &a, v2 &b) { gk::landed(a, b); }
};

// A plain (default-policy) load through an address-space-1 pointer: where the compiler
// cannot prove a pointer global (pointers selected per pass from small arrays) it emits
// FLAT loads, and waited for each before issuing the next inside an unrolled batch.
__device__ __forceinline__ double2 ldg(const double2 *p) {
    const d2v t = *(const __attribute__((address_space(1))) d2v *)p;
    return double2{t.x, t.y};
}

template <int VEC>
__device__ __forceinline__ void ld_vec(const double *p, bool ok, double (&v)[VEC]) {
    if (ok) {
        if constexpr (VEC == 2) {
            const double2 t = *reinterpret_cast<const double2 *>(p);
            v[0] = t.x;
            v[1] = t.y;
        } else {
            v[0] = p[0];
        }
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.0;
    }
}

template <int VEC>
__device__ __forceinline__ void st_vec(double *p, const double (&v)[VEC]) {
    if constexpr (VEC == 2) {
        *reinterpret_cast<double2 *>(p) = double2{v[0], v[1]};
    } else {
        p[0] = v[0];
    }
}

// Fused reductions of a pass: none, <y, vdot>, or <y, y>.
enum { ACC_NONE = 0, ACC_DOT = 1, ACC_NORM = 2 };

// What one k_proj launch does (gk_step_kernels.hpp; the callers of gk_host.hpp's proj name it).
enum { PJ_DOT = 0, PJ_AXPY = 1, PJ_AXPY_DOT = 2, PJ_AXPY_NORM = 3 };

constexpr int GCMAX = 128;  // most columns of a Gram diagnostic (k_gram; sizes the pinned read-back buffer)

// --------------------------------------------------------------------------
// Reference-order dots for the orthogonality diagnostics (gmres_mgsr.f90:414-420,
// gmres_hh.f90:568-593).  Fortran dot_product is ONE running sum
// h = h + a(k)*b(k), k = 1..n.  Both diagnostics measure rounding noise, and
// the reference's figure is dominated by that running sum's own rounding, so
// the device evaluates them the same way: one lane per dot, k in order,
// multiply then add (-ffp-contract=off) -- bit-identical to the reference's
// formula on the same basis.  n dependent adds per lane: slow by design, run
// once per solve (the tree-reduced k_gram is the fast alternative).  Its two
// kernels: k_seqdot_pairs (gk_step_kernels.hpp), k_hh_rebuild_dot (gk_hh_kernels.hpp).
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

// A kernel launched with `lds` bytes of dynamic LDS needs that size allowed first.
// hipFuncSetAttribute is per device: memo[ATTR_DEVS] (one per kernel instantiation)
// remembers the size set on each.  Returns a hipError_t (hipErrorInvalidDevice for a
// device id outside the memo).
constexpr int ATTR_DEVS = 64;
inline hipError_t ensure_dyn_lds(const void *kernel, int dev, int lds, std::atomic<int> *memo) {
    if (dev < 0 || dev >= ATTR_DEVS) return hipErrorInvalidDevice;
    if (lds > 0 && memo[dev].load() < lds) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        memo[dev] = lds;
    }
    return hipSuccess;
}

}  // namespace gk
