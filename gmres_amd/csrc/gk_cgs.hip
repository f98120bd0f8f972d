// gk_cgs.hip -- the CGS2 Arnoldi step's kernels for gfx950 (gk_cgs.hpp).
//
// All three are HBM-bandwidth bound and follow gk_step_kernels.hpp's rules: double2 accesses
// along the vector, one partial per workgroup into a fixed slab that the next launch
// re-reduces in a fixed order, the odd-length tail element on thread 0 of workgroup 0,
// and -ffp-contract=off so that every element-wise expression is the stated one.
//
// Bytes per unknown and sweep: the dots read the j columns once and w once per batch of KB
// columns, 8 (j + ceil(j / KB)); the AXPY reads the j columns and w and writes w, 8 (j + 2).
#include "gk_cgs.hpp"

namespace gk {

// slab[(k0 + k) * gridDim.x + blockIdx.x] = this workgroup's share of <w, V_{k0+k}>,
// k0 = blockIdx.y * KB, k < min(KB, j - k0).  A thread keeps KB accumulators and, per trip,
// has one double2 of w and KB column double2 in flight (KB + 1 independent 16-byte loads).
template <int KB, bool NT, bool FULL>
__device__ __forceinline__ void cgs_dots_walk(const double2 *__restrict__ W2, const double2 *__restrict__ C2, i64 ld2,
                                              int kb, i64 n2, double (&acc)[KB]) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
        const double2 wv = W2[e];
        double2 cv[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) cv[k] = (FULL || k < kb) ? ldv<NT>(C2 + (i64)k * ld2 + e) : double2{0.0, 0.0};
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            acc[k] = acc[k] + wv.x * cv[k].x;
            acc[k] = acc[k] + wv.y * cv[k].y;
        }
    }
}

template <int KB, bool NT>
__global__ __launch_bounds__(TPB) void k_cgs_dots(const double *__restrict__ w, const double *__restrict__ V, i64 ld,
                                                  int j, i64 n, double *__restrict__ slab) {
    __shared__ double sm[KB][WAVES];
    const int k0 = blockIdx.y * KB;
    const int kb = min(KB, j - k0);  // the last batch may be ragged
    const double *__restrict__ C = V + (i64)k0 * ld;
    const double2 *__restrict__ W2 = reinterpret_cast<const double2 *>(w);
    const double2 *__restrict__ C2 = reinterpret_cast<const double2 *>(C);
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    if (kb == KB)
        cgs_dots_walk<KB, NT, true>(W2, C2, ld >> 1, kb, n >> 1, acc);
    else
        cgs_dots_walk<KB, NT, false>(W2, C2, ld >> 1, kb, n >> 1, acc);
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd-length tail element
        const double x = w[n - 1];
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < kb) acc[k] = acc[k] + x * C[(i64)k * ld + n - 1];
    }
    // the KB block sums at once: wave sums, then the waves in a fixed order
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) sm[k][wid] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < kb) {
        double r = sm[threadIdx.x][0];
#pragma unroll
        for (int q = 1; q < WAVES; ++q) r += sm[threadIdx.x][q];
        slab[(i64)(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = r;
    }
}

// s[k] = sum_b slab[k][b], b in reduce_slab's fixed order; one workgroup per column.
__global__ __launch_bounds__(TPB) void k_cgs_reduce(const double *__restrict__ slab, int G, double *__restrict__ s) {
    __shared__ double sm[WAVES];
    const double v = reduce_slab(slab + (i64)blockIdx.x * G, G, sm);
    if (threadIdx.x == 0) s[blockIdx.x] = v;
}

// w_e = ((w_e - s_0 V_0,e) - s_1 V_1,e) .. - s_{j-1} V_{j-1},e with s staged in j doubles of
// dynamic LDS; workgroup 0 also folds s into the step's Hessenberg column (after the
// all-reduce, so N ranks accumulate the rank total).  NORM: the partial of ||w||^2 of the
// values written goes to pout[blockIdx.x] for the closing scale.
constexpr int AXB = 8;  // column double2 a thread of k_cgs_axpy loads per batch

template <bool NORM, bool NT>
__global__ __launch_bounds__(TPB) void k_cgs_axpy(double *__restrict__ w, const double *__restrict__ V, i64 ld, int j,
                                                  i64 n, const double *__restrict__ s, double *__restrict__ hs,
                                                  int hstore, double *__restrict__ pout) {
    extern __shared__ double sh[];
    __shared__ double sm[WAVES];
    for (int k = threadIdx.x; k < j; k += TPB) {
        const double v = s[k];
        sh[k] = v;
        if (blockIdx.x == 0) hs[k] = (hstore ? 0.0 : hs[k]) + v;
    }
    __syncthreads();
    const i64 n2 = n >> 1, ld2 = ld >> 1;
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(w);
    const double2 *__restrict__ V2 = reinterpret_cast<const double2 *>(V);
    const i64 stride = (i64)gridDim.x * TPB;
    double acc = 0.0;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
        double2 wv = W2[e];
        int k = 0;
        for (; k + AXB <= j; k += AXB) {  // AXB column loads in flight, applied in ascending k
            double2 v[AXB];
#pragma unroll
            for (int u = 0; u < AXB; ++u) v[u] = ldv<NT>(V2 + (i64)(k + u) * ld2 + e);
#pragma unroll
            for (int u = 0; u < AXB; ++u) {
                const double sk = sh[k + u];
                wv.x = wv.x - sk * v[u].x;
                wv.y = wv.y - sk * v[u].y;
            }
        }
        for (; k < j; ++k) {
            const double2 v = ldv<NT>(V2 + (i64)k * ld2 + e);
            const double sk = sh[k];
            wv.x = wv.x - sk * v.x;
            wv.y = wv.y - sk * v.y;
        }
        W2[e] = wv;
        if (NORM) {
            acc = acc + wv.x * wv.x;
            acc = acc + wv.y * wv.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd-length tail element
        double x = w[n - 1];
        for (int k = 0; k < j; ++k) x = x - sh[k] * V[(i64)k * ld + n - 1];
        w[n - 1] = x;
        if (NORM) acc = acc + x * x;
    }
    if (NORM) {
        const double t = block_sum(acc, sm);
        if (threadIdx.x == 0) pout[blockIdx.x] = t;
    }
}

template <int KB>
static hipError_t launch_dots(bool nt, int G, const double *w, const double *V, i64 ld, int j, i64 n, double *slab,
                              hipStream_t st) {
    const dim3 g(G, (j + KB - 1) / KB);
    if (nt)
        k_cgs_dots<KB, true><<<g, TPB, 0, st>>>(w, V, ld, j, n, slab);
    else
        k_cgs_dots<KB, false><<<g, TPB, 0, st>>>(w, V, ld, j, n, slab);
    return hipGetLastError();
}

hipError_t cgs_dots(int kb, bool nt, int G, const double *w, const double *V, i64 ld, int j, i64 n, double *slab,
                    hipStream_t st) {
    if (j < 1 || G < 1 || G > NPMAX || (ld & 1)) return hipErrorInvalidValue;
    return kb == 16 ? launch_dots<16>(nt, G, w, V, ld, j, n, slab, st) : launch_dots<8>(nt, G, w, V, ld, j, n, slab, st);
}

hipError_t cgs_reduce(const double *slab, int G, int j, double *s, hipStream_t st) {
    if (j < 1 || G < 1 || G > NPMAX) return hipErrorInvalidValue;
    k_cgs_reduce<<<j, TPB, 0, st>>>(slab, G, s);
    return hipGetLastError();
}

hipError_t cgs_axpy(bool norm, bool nt, int G, double *w, const double *V, i64 ld, int j, i64 n, const double *s,
                    double *hs, int hstore, double *pout, hipStream_t st) {
    if (j < 1 || G < 1 || G > NPMAX || (ld & 1)) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)j;  // sized from j (far below the 64 KiB a launch may ask for)
    if (lds > 48 * 1024) return hipErrorInvalidValue;
    if (norm) {
        if (nt)
            k_cgs_axpy<true, true><<<G, TPB, lds, st>>>(w, V, ld, j, n, s, hs, hstore, pout);
        else
            k_cgs_axpy<true, false><<<G, TPB, lds, st>>>(w, V, ld, j, n, s, hs, hstore, pout);
    } else {
        if (nt)
            k_cgs_axpy<false, true><<<G, TPB, lds, st>>>(w, V, ld, j, n, s, hs, hstore, pout);
        else
            k_cgs_axpy<false, false><<<G, TPB, lds, st>>>(w, V, ld, j, n, s, hs, hstore, pout);
    }
    return hipGetLastError();
}

}  // namespace gk
