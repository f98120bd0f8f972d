// gk_cb.hip -- the MGS-R step on an FP32-compressed Krylov basis (gk_cb.hpp;
// gk_set_basis_precision GK_BASIS_F32): the resident step k_mgs_wcb, its planner and
// launcher, and the two launch-path kernels that exist on float columns only (the scale
// that writes the column, the widening copy).  The launch path's projection, x update and
// Gram are the float instantiations of gk_step_kernels.hpp's k_proj / k_update_x / k_gram.
//
// The basis is STORED in FP32; w, every dot, every AXPY, the H column and x stay FP64.
// A column element is widened exactly on load, and the FP64 expressions and their order
// are k_mgs_wres's / k_proj's (w = w - h a; acc = acc + w.x b.x, then .y).  The new
// column is float(w_i / h): the division in FP64, one round-to-nearest-even conversion,
// 0 when h = 0; the same value widened goes to vjw, which the operator stage reads.
// A projection then moves 8 B per unknown of the resident part instead of 16.
#include <algorithm>

#include "../../include/gmres_hip.h"
#include "gk_cb.hpp"
#include "gk_res.hpp"
#include "gk_resident.hpp"

namespace gk {

// four floats (16 bytes, 16-B aligned) of a column (two: ldf / landed of gk_common.hpp)
typedef float f4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ f4v ldf4(const float2 *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(reinterpret_cast<const f4v *>(p));
    else
        return *reinterpret_cast<const f4v *>(p);
}
__device__ __forceinline__ void landed(f4v &a, f4v &b) { asm volatile("" : "+v"(a), "+v"(b)); }

// the stored form of one new column element and what every later reader sees of it: res_unit
// (gk_res.hpp, which states the zero-norm rule) rounded once to FP32
__device__ __forceinline__ float cb_round(double w, double h) { return h != 0.0 ? (float)(w / h) : 0.0f; }

// --------------------------------------------------------------------------
// Resident MGS-R step on float columns: k_mgs_wres's batch (non-pipelined) pass --
// one 256-thread workgroup per CU pinned by its dynamic LDS, w in RW register chunks
// plus LW LDS chunks of 256 double2, the resident prefix spread evenly (r2e / l2e), the
// streamed remainder handed out from the last workgroup down, the odd-n tail element,
// the H column in LDS (WO_HMAX), the in-launch all-gather of gk_res.hpp unchanged, the
// L2 touch of the next dot column during the wait.  Per PAIR of adjacent chunks a lane
// loads one float4 of V_i (non-temporal) and one of V_q (default policy: the next pass's
// V_i) -- 16-B loads, 1 KiB contiguous per wave; an unpaired last chunk one float2 each.
// The w layout that goes with the pairs is the kernel's own (it loads and stores w
// itself).  The closing writes the FP32 column and vjw.
// Measured at 4096^2, m = 95 (tools/cb_bench.py, profiles/r09): 8-B loads in batches of 8
// chunks 27.6 us per projection pass (305.9 it/s), batches of 12 / 16 25.7 / 25.5 us
// (327.1 / 328.4 it/s, ab_cb_batch_depth_8B_loads.jsonl), the pairs in batches of 16
// 23.6 us (345.1 it/s); the FP64 step beside them 29.3 us (273 it/s).
// --------------------------------------------------------------------------
#ifndef GK_CB_WB
#define GK_CB_WB 16
#endif
constexpr int CB_WB = GK_CB_WB;  // chunks per column per batch in flight per thread
// touched chunks per workgroup and the pacing of the touch loads: k_mgs_wres's batch-pass
// values (a touched chunk is 16 lines of 128 B here, half of the FP64 kernel's 32)
#ifndef GK_CB_TOUCH
#define GK_CB_TOUCH 28
#endif
#ifndef GK_CB_TOUCH_PACE
#define GK_CB_TOUCH_PACE 24
#endif
constexpr int CB_TOUCH = GK_CB_TOUCH, CB_TOUCH_PACE = GK_CB_TOUCH_PACE;

struct CbArgs {
    ResArgs r;        // w, pin, hs, hcopy, the all-gather words, j, n, nres2, r2e, l2e, ld (V / vout unused)
    const float *F;   // FP32 basis, column stride r.ld floats
    float *fout;      // its column j + 1 (0-based j)
    double *vjw;      // the same column widened
};

template <int RW, int LW, int WBT>
__global__ __launch_bounds__(CB_WT, 1) void k_mgs_wcb(CbArgs ca) {
    constexpr int WT = CB_WT;
    extern __shared__ double2 lw[];  // [LW][WT]
    __shared__ double sm[WT / 64];
    __shared__ double bc[1];
    __shared__ int okf;
    __shared__ int xdone;  // the exchange in progress has completed
    __shared__ double hsh[WO_HMAX];  // H(1:j, j)
    const ResArgs &a = ca.r;
    const int t = threadIdx.x;
    constexpr int PACE = CB_TOUCH_PACE, TCH = CB_TOUCH;
    const int j = a.j, np = 2 * j;
    const i64 n2 = a.n >> 1, ld2 = a.ld >> 1;  // float2 / double2 per column
    const i64 nch = a.nres2 / WT;
    const i64 bq = blockIdx.x;  // chunk range of this workgroup
    const i64 c0 = bq * a.r2e, cend = c0 + a.r2e < nch ? c0 + a.r2e : nch;
    const i64 l0 = (i64)gridDim.x * a.r2e + bq * a.l2e, lend = l0 + a.l2e < nch ? l0 + a.l2e : nch;
    const float2 *__restrict__ F2 = reinterpret_cast<const float2 *>(ca.F);
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(a.w);
    ResClock clk;
    clk.start(a.stamps);
    int touch_sink = 0;
    const i64 sstride = (i64)gridDim.x * WT;
    const i64 sbase = a.nres2 + (i64)res_stream_wg() * WT + t;
    const bool tail = (a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0;  // the odd-length tail element
    // Two adjacent chunks of a workgroup's range are one PAIR where both are held (an odd
    // count leaves the last chunk single): a lane then owns 4 consecutive unknowns' worth
    // of each column, double2 2t and 2t + 1 of the pair's 512, and loads them as ONE 16-B
    // float4 per column instead of two 8-B float2 -- half the load instructions of a pass
    // (25.5 -> 23.6 us per projection at 4096^2, profiles/r09).  The kernel
    // loads and stores w itself, so the layout is its own: e2r / e2l give the double2 index
    // lane t holds in register / LDS chunk k.
    auto pair_r = [&](int k) { return (k | 1) < RW && c0 + (k | 1) < cend; };
    auto pair_l = [&](int k) { return (k | 1) < LW && l0 + (k | 1) < lend; };
    auto e2r = [&](int k) { return pair_r(k) ? (c0 + (k & ~1)) * WT + 2 * t + (k & 1) : (c0 + k) * WT + t; };
    auto e2l = [&](int k) { return pair_l(k) ? (l0 + (k & ~1)) * WT + 2 * t + (k & 1) : (l0 + k) * WT + t; };
    double2 wr[RW];
#pragma unroll
    for (int k = 0; k < RW; ++k) wr[k] = (c0 + k < cend) ? W2[e2r(k)] : double2{0.0, 0.0};
    for (int k = 0; k < LW; ++k)
        if (l0 + k < lend) lw[k * WT + t] = W2[e2l(k)];
    // acc += the closing reduction of one element pair: <w, V_q> or ||w||^2
    auto red = [&](double &acc, const double2 &v, float bx, float by, bool dot) {
        if (dot) {
            acc = acc + v.x * (double)bx;
            acc = acc + v.y * (double)by;
        } else {
            acc = acc + v.x * v.x;
            acc = acc + v.y * v.y;
        }
    };
    // One pass over the slab: w -= ch V_i, then <w, V_q> (dot) or ||w||^2.  Returns this
    // thread's partial.
    static_assert(WBT % 2 == 0, "a batch holds whole chunk pairs");
    auto pass = [&](double ch, int i, int q, bool dot) -> double {
        const float2 *__restrict__ A2 = F2 + (i64)i * ld2;
        const float2 *__restrict__ B2 = F2 + (i64)q * ld2;
        double acc = 0.0;
        // the float4 (pair) or float2 (single chunk: .xy) of a column that lane t owns in the
        // chunk(s) starting at chunk c
        auto ld4 = [&](const float2 *C2, i64 c, bool pair, auto nt) -> f4v {
            constexpr bool NT = decltype(nt)::value;
            if (pair) return ldf4<NT>(C2 + c * WT + 2 * t);
            const f2v v = ldf<NT>(C2 + c * WT + t);
            return f4v{v.x, v.y, 0.0f, 0.0f};
        };
        // registers: batches of WBT chunks = WBT / 2 pairs, both columns in flight (k0 a
        // constant once unrolled)
        auto rbatch = [&](const int k0) {
            f4v av[WBT / 2], bv[WBT / 2];
#pragma unroll
            for (int u = 0; u < WBT / 2; ++u) {
                const int k = k0 + 2 * u;
                if (k < RW && c0 + k < cend) {
                    av[u] = ld4(A2, c0 + k, pair_r(k), std::true_type{});
                    if (dot) bv[u] = ld4(B2, c0 + k, pair_r(k), std::false_type{});
                }
            }
#pragma unroll
            for (int u = 0; u < WBT / 2; ++u) {
                const int k = k0 + 2 * u, k1 = k + 1 < RW ? k + 1 : k;
                if (k < RW && c0 + k < cend) {
                    landed(av[u], bv[u]);
                    wr[k].x = wr[k].x - ch * (double)av[u].x;
                    wr[k].y = wr[k].y - ch * (double)av[u].y;
                    red(acc, wr[k], bv[u].x, bv[u].y, dot);
                    if (pair_r(k)) {
                        wr[k1].x = wr[k1].x - ch * (double)av[u].z;
                        wr[k1].y = wr[k1].y - ch * (double)av[u].w;
                        red(acc, wr[k1], bv[u].z, bv[u].w, dot);
                    }
                }
            }
        };
        // LDS: the same, w from / to LDS
        auto lbatch = [&](const int k0) {
            f4v av[WBT / 2], bv[WBT / 2];
#pragma unroll
            for (int u = 0; u < WBT / 2; ++u) {
                const int k = k0 + 2 * u;
                if (k < LW && l0 + k < lend) {
                    av[u] = ld4(A2, l0 + k, pair_l(k), std::true_type{});
                    if (dot) bv[u] = ld4(B2, l0 + k, pair_l(k), std::false_type{});
                }
            }
#pragma unroll
            for (int u = 0; u < WBT / 2; ++u) {
                const int k = k0 + 2 * u;
                if (k < LW && l0 + k < lend) {
                    landed(av[u], bv[u]);
                    double2 wv = lw[k * WT + t];
                    wv.x = wv.x - ch * (double)av[u].x;
                    wv.y = wv.y - ch * (double)av[u].y;
                    lw[k * WT + t] = wv;
                    red(acc, wv, bv[u].x, bv[u].y, dot);
                    if (pair_l(k)) {
                        double2 wv1 = lw[(k + 1) * WT + t];
                        wv1.x = wv1.x - ch * (double)av[u].z;
                        wv1.y = wv1.y - ch * (double)av[u].w;
                        lw[(k + 1) * WT + t] = wv1;
                        red(acc, wv1, bv[u].z, bv[u].w, dot);
                    }
                }
            }
        };
#pragma unroll
        for (int k0 = 0; k0 < RW; k0 += WBT) rbatch(k0);
        for (int k0 = 0; k0 < LW; k0 += WBT) lbatch(k0);
        for (i64 e0 = sbase; e0 < n2; e0 += 2 * sstride) {  // streamed part: w from / to HBM
            double2 wv[2];
            f2v av[2], bv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    wv[u] = W2[e];
                    av[u] = ldf<true>(A2 + e);
                    if (dot) bv[u] = ldf<false>(B2 + e);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    landed(av[u], bv[u]);
                    wv[u].x = wv[u].x - ch * (double)av[u].x;
                    wv[u].y = wv[u].y - ch * (double)av[u].y;
                    W2[e] = wv[u];
                    red(acc, wv[u], bv[u].x, bv[u].y, dot);
                }
            }
        }
        if (tail) {
            const i64 e = a.n - 1;
            const double x = a.w[e] - ch * (double)ca.F[(i64)i * a.ld + e];
            a.w[e] = x;
            acc = dot ? acc + x * (double)ca.F[(i64)q * a.ld + e] : acc + x * x;
        }
        return acc;
    };
    // all-gather of the partials: the same h in every workgroup; waves 1..3 meanwhile pull
    // the first TCH register chunks of column touch_col (the next pass's dot column, the
    // one that comes from HBM) into L2, one dword load per 128-B line into a sink register
    int xi = 0;
    auto reduce = [&](double acc, double &h, int touch_col) -> bool {
        clk.passed(a.stamps);
        acc = wave_sum(acc);
        if ((t & 63) == 0) sm[t >> 6] = acc;
        if (PACE > 0 && t == 0) xdone = 0;
        __syncthreads();
        if (t < 64) {
            res_exchange<WT / 64, true, RES_POLL_SLEEP>(a, xi, sm, bc, &okf);
            if (PACE > 0 && t == 0) *(volatile int *)&xdone = 1;
        } else if (TCH > 0 && touch_col >= 0) {
            // a chunk of a float column is 16 lines; all loads land in one sink register,
            // drained below before anything can reuse it
            const i64 nc = cend - c0;
            const i64 lines = (i64)16 * (nc < TCH ? (nc > 0 ? nc : 0) : TCH);
            const char *base = reinterpret_cast<const char *>(F2 + (i64)touch_col * ld2 + c0 * WT);
            res_touch<PACE>(base, lines, t - 64, WT - 64, &xdone, touch_sink);
        }
        __syncthreads();
        if constexpr (TCH > 0) asm volatile("s_waitcnt vmcnt(0)" : : "v"(touch_sink) : "memory");
        ++xi;
        h = bc[0];
        clk.waited(a.stamps);
        return okf != 0;
    };
    // the first dot <w, V(:,1)> from the operator launch's partial slab
    double h;
    {
        double s = 0.0;
        for (int k = t; k < a.npin; k += WT) s += a.pin[k];
        s = wave_sum(s);
        if ((t & 63) == 0) sm[t >> 6] = s;
        __syncthreads();
        h = sm[0];
#pragma unroll
        for (int w = 1; w < WT / 64; ++w) h += sm[w];
        __syncthreads();
    }
    bool ok = true;
    for (int p = 0; p < np && ok; ++p) {
        const int i = p % j;
        const bool dot = p < np - 1;
        if (blockIdx.x == 0 && t == 0) hsh[i] = (p < j ? 0.0 : hsh[i]) + h;  // H(i,j) (+)= h
        const double acc = pass(h, i, (p + 1) % j, dot);
        ok = reduce(acc, h, p + 2 < np ? (p + 2) % j : -1);
    }
    if (!ok) return;  // uniform per workgroup; *err is set
    // V(:,j+1) = float(w / ||w||), and the same values widened for the operator stage
    const double hn = sqrt(h);
    float2 *__restrict__ O2 = reinterpret_cast<float2 *>(ca.fout);
    double2 *__restrict__ J2 = reinterpret_cast<double2 *>(ca.vjw);
    auto store = [&](i64 e, const double2 &v) {
        const float2 f{cb_round(v.x, hn), cb_round(v.y, hn)};
        O2[e] = f;
        J2[e] = double2{(double)f.x, (double)f.y};
    };
#pragma unroll
    for (int k = 0; k < RW; ++k)
        if (c0 + k < cend) store(e2r(k), wr[k]);
    for (int k = 0; k < LW; ++k)
        if (l0 + k < lend) store(e2l(k), lw[k * WT + t]);
    for (i64 e = sbase; e < n2; e += sstride) store(e, W2[e]);
    if (tail) {
        const float f = cb_round(a.w[a.n - 1], hn);
        ca.fout[a.n - 1] = f;
        ca.vjw[a.n - 1] = (double)f;
    }
    clk.finish(a.stamps, RES_MGS);
    res_store_hcol<WT>(a, hsh, j, hn);
}

// static LDS of k_mgs_wcb: sm, bc, okf, xdone, hsh
constexpr int CB_LDS_STATIC = (CB_WT / 64 + 1 + WO_HMAX) * (int)sizeof(double) + 2 * (int)sizeof(int);
constexpr int CB_LDS_DYN = CB_LW * CB_WT * (int)sizeof(double2);
static_assert(CB_LDS_STATIC + CB_LDS_DYN <= 160 * 1024, "k_mgs_wcb: LDS of one CU");
static_assert(CB_LDS_DYN > 80 * 1024, "k_mgs_wcb: the dynamic LDS must pin one workgroup per CU");

// ---------------------------------------------------------------- planner ---
void plan_cb(i64 nloc, int cus, int share, int m, CbPlan &p) {
    p = CbPlan{};
    p.G = std::max(1, std::min(RGMAX, cus / std::max(1, share)));
    const i64 n2 = nloc / 2;
    res_spread(n2, CB_WT, p.G, CB_RW, CB_LW, p.r2e, p.l2e, p.nres2);
    p.nstream2 = n2 - p.nres2;
    p.lds = CB_LDS_DYN;
    p.on = m + 1 <= WO_HMAX;  // the H column: WO_HMAX entries of LDS
}

void cb_plan_info(const CbPlan &p, long long *info) {
    info[CPI_G] = p.G;
    info[CPI_RW] = CB_RW;
    info[CPI_LW] = CB_LW;
    info[CPI_R2E] = p.r2e;
    info[CPI_L2E] = p.l2e;
    info[CPI_LDS] = p.lds;
    info[CPI_NRES2] = p.nres2;
    info[CPI_STREAM2] = p.nstream2;
    info[CPI_ON] = p.on ? 1 : 0;
    info[CPI_LDS_STATIC] = CB_LDS_STATIC;
}

// --------------------------------------------------------------- launcher ---
int cb_launch(const CbPlan &p, const ResArgs &a, float *F, double *vjw, int dev, hipStream_t st, std::string &msg) {
    if (!p.on || p.r2e > CB_RW || p.l2e > CB_LW || p.G < 1 || p.G > RGMAX || a.j < 1 || a.j + 1 > WO_HMAX ||
        a.nres2 != p.nres2 || a.nranks != 1 || (a.nres2 % CB_WT) != 0 || a.nres2 > a.n / 2 ||
        a.nres2 > (i64)p.G * (p.r2e + p.l2e) * CB_WT)
        return fail(msg, GK_ERR_STATE, "compressed-basis step: plan (%d + %d chunks on %d workgroups) does not fit", p.r2e,
                    p.l2e, p.G);
    static std::atomic<int> attr[ATTR_DEVS];
    const int e = dyn_lds(reinterpret_cast<const void *>(&k_mgs_wcb<CB_RW, CB_LW, CB_WB>), dev, p.lds, attr, msg);
    if (e != GK_OK) return e;
    CbArgs ca{};
    ca.r = a;
    ca.F = F;
    ca.fout = F + (i64)a.j * a.ld;
    ca.vjw = vjw;
    k_mgs_wcb<CB_RW, CB_LW, CB_WB><<<p.G, CB_WT, p.lds, st>>>(ca);
    return launched("compressed-basis step", msg);
}

// k_scale writing the float column: out = float(w / h), h = sqrt(sum(pin)); the same
// values widened to vjw and (cycle start: column 1) to v1w.  hslot / hcopy as k_scale.
__global__ __launch_bounds__(TPB) void k_scale_cb(float *__restrict__ out, double *__restrict__ vjw,
                                                  double *__restrict__ v1w, const double *__restrict__ w,
                                                  const double *__restrict__ pin, int npin,
                                                  double *__restrict__ hslot, i64 n, double *__restrict__ hcopy,
                                                  const double *__restrict__ hsrc, int ncopy) {
    __shared__ double sm[WAVES];
    const double h = sqrt(reduce_slab(pin, npin, sm));
    if (hslot != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *hslot = h;
    if (hcopy != nullptr && blockIdx.x == 0) {
        for (int k = threadIdx.x; k < ncopy; k += TPB) hcopy[k] = hsrc[k];
        if (threadIdx.x == 0) hcopy[ncopy] = h;
    }
    const i64 n2 = n >> 1;
    const double2 *__restrict__ W2 = reinterpret_cast<const double2 *>(w);
    float2 *__restrict__ O2 = reinterpret_cast<float2 *>(out);
    double2 *__restrict__ J2 = reinterpret_cast<double2 *>(vjw);
    double2 *__restrict__ I2 = reinterpret_cast<double2 *>(v1w);
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n2; e += stride) {
        const double2 v = W2[e];
        const float2 f{cb_round(v.x, h), cb_round(v.y, h)};
        const double2 d{(double)f.x, (double)f.y};
        O2[e] = f;
        J2[e] = d;
        if (v1w != nullptr) I2[e] = d;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const float f = cb_round(w[n - 1], h);
        out[n - 1] = f;
        vjw[n - 1] = (double)f;
        if (v1w != nullptr) v1w[n - 1] = (double)f;
    }
}

hipError_t cb_scale(int blocks, float *out, double *vjw, double *v1w, const double *w, const double *pin, int npin,
                    double *hslot, i64 n, double *hcopy, const double *hsrc, int ncopy, hipStream_t st) {
    k_scale_cb<<<blocks, TPB, 0, st>>>(out, vjw, v1w, w, pin, npin, hslot, n, hcopy, hsrc, ncopy);
    return hipGetLastError();
}

__global__ __launch_bounds__(TPB) void k_widen_cb(double *__restrict__ out, const float *__restrict__ in, i64 n) {
    const i64 stride = (i64)gridDim.x * TPB;
    for (i64 e = (i64)blockIdx.x * TPB + threadIdx.x; e < n; e += stride) out[e] = (double)in[e];
}

hipError_t cb_widen(int blocks, double *out, const float *in, i64 n, hipStream_t st) {
    k_widen_cb<<<blocks, TPB, 0, st>>>(out, in, n);
    return hipGetLastError();
}

}  // namespace gk

