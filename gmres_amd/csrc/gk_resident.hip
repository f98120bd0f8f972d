// gk_resident.hip -- the resident MGS-R / Householder step (gk_resident.hpp): the
// strict kernels k_mgs_res / k_mgs_wres / k_mgs_wpc, the planner that picks one
// for a slab, and their launchers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>

#include "../../include/gmres_hip.h"
#include "gk_blk.hpp"
#include "gk_res.hpp"
#include "gk_resident.hpp"

namespace gk {

// R2: register-resident double2 per data thread (w, and the running column);
// L2: LDS-resident double2 of w per data thread (its two columns stream);
// PF: the next column is loaded into a third register array before the wait;
// CW: wave 0 holds no data and only runs the exchange, so its polls never wait
//     behind prefetch loads (vmcnt retires in issue order).
template <int R2, int L2, bool PF, bool NT, bool CW, int MODE>
__global__ __launch_bounds__(RT, 2) void k_mgs_res(ResArgs a) {
    extern __shared__ double2 lw[];  // L2 > 0: [L2][DT] LDS-resident part of w
    __shared__ double sm[RWAVES];
    __shared__ double bc[1];
    __shared__ int okf;
    __shared__ double hsh[RHMAX + 1];
    constexpr int RB = PF ? R2 : 1;
    constexpr int DT = CW ? RT - 64 : RT;  // data threads per workgroup
    const int t = threadIdx.x;
    const bool data = !CW || t >= 64;
    const int td = CW ? t - 64 : t;
    constexpr int mode = MODE;
    const int j = a.j, np = res_np(mode, j);
    const i64 n2 = a.n >> 1, ld2 = a.ld >> 1;
    const i64 tail0 = mode == RES_HH_UP ? a.tail0 : 0;
    // Resident layout in chunks of DT double2 (data thread td holds element td
    // of each): registers hold chunks b*R2 + k (k < R2), LDS chunks G*R2 + b*L2
    // + k (k < L2); a chunk is resident when it lies below nres2 (a multiple of
    // DT), so the test is uniform and every address is a uniform base + td*16.
    // [nres2, n2) streams through w in HBM as in k_proj.
    const i64 nch = a.nres2 / DT;
    const i64 c0 = (i64)blockIdx.x * a.r2e, cend = c0 + a.r2e < nch ? c0 + a.r2e : nch;
    const i64 l0 = (i64)gridDim.x * a.r2e + (i64)blockIdx.x * a.l2e, lend = l0 + a.l2e < nch ? l0 + a.l2e : nch;
    const double2 *__restrict__ V2 = reinterpret_cast<const double2 *>(a.V);
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(a.w);
    auto colchunk = [&](int col, i64 c) { return V2 + (i64)col * ld2 + c * DT; };
    double2 wr[R2], xa[R2], xb[RB];
#pragma unroll
    for (int k = 0; k < R2; ++k) {  // zeros past nres2: they add exact zeros to every dot
        wr[k] = xa[k] = double2{0.0, 0.0};
        if constexpr (PF) xb[k] = double2{0.0, 0.0};
        if (data && c0 + k < cend) {
            wr[k] = W2[(c0 + k) * DT + td];
            xa[k] = colchunk(res_col(mode, j, 0), c0 + k)[td];              // AXPY partner of projection 0
            if constexpr (PF) xb[k] = colchunk(res_col(mode, j, 1), c0 + k)[td];  // its dot partner
        }
    }
    if constexpr (L2 > 0) {
        for (int k = 0; k < L2; ++k)
            if (data && l0 + k < lend) lw[k * DT + td] = W2[(l0 + k) * DT + td];
    }
    const i64 sstride = (i64)gridDim.x * DT;
    const i64 sbase = a.nres2 + (i64)res_stream_wg() * DT + td;
    ResClock clk;
    clk.start(a.stamps);
    int xi = 0;  // exchange index
    double h;
    bool ok = true;
    if (mode == RES_HH_DOWN) {  // the pre-dot <v, V_col(0)> (xa holds V_col(0))
        const int q = res_col(mode, j, 0);
        const double2 *__restrict__ B2 = V2 + (i64)q * ld2;
        double acc = 0.0;
        if (a.unit_known) {  // <e_u, P_q> = P_q(u): the one nonzero product, as the full sum gives it
            if (blockIdx.x == 0 && t == 0 && a.unit_e >= 0) acc = a.V[(i64)q * a.ld + a.unit_e];
        } else if (data) {
#pragma unroll
            for (int k = 0; k < R2; ++k) {
                acc = acc + wr[k].x * xa[k].x;
                acc = acc + wr[k].y * xa[k].y;
            }
            if constexpr (L2 > 0) {
                for (int k = 0; k < L2; ++k)
                    if (l0 + k < lend) {
                        const double2 wv = lw[k * DT + td], bv = ldv<NT>(B2 + (l0 + k) * DT + td);
                        acc = acc + wv.x * bv.x;
                        acc = acc + wv.y * bv.y;
                    }
            }
            for (i64 e = sbase; e < n2; e += sstride) {
                const double2 wv = W2[e], bv = ldv<NT>(B2 + e);
                acc = acc + wv.x * bv.x;
                acc = acc + wv.y * bv.y;
            }
            if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && td == 0) acc = acc + a.w[a.n - 1] * a.V[(i64)q * a.ld + a.n - 1];
        }
        acc = wave_sum(acc);
        if ((t & 63) == 0) sm[t >> 6] = acc;
        __syncthreads();
        if (t < 64) res_exchange<RWAVES, MODE == RES_MGS, RES_POLL_SLEEP_SMALL>(a, xi, sm, bc, &okf);
        __syncthreads();
        ++xi;
        h = bc[0];
        ok = okf != 0;
    } else {
        double s = 0.0;
        for (int k = t; k < a.npin; k += RT) s += a.pin[k];
        h = block_sum_rt(s, sm);
        ok = res_pin_fold(a, h, bc, &okf);
    }
    // Projection p: i = p mod j, AXPY w -= h V_i (h = the dot of p), then the
    // dot of projection p+1 with V_q, q = (p+1) mod j -- or ||w||^2 after the
    // last one.  X holds V_i; PF: Y holds V_q (prefetched), and X <- the dot
    // partner of p+1 is loaded before the wait.
    auto proj = [&](int p, auto &X, auto &Y) -> bool {
        const int i = res_col(mode, j, p);
        const bool last = p == np - 1;
        const int q = res_col(mode, j, p + 1);
        const int kind = !last ? RK_DOT : (mode == RES_HH_DOWN ? RK_NONE : RK_NORM);
        if (mode == RES_MGS && blockIdx.x == 0 && t == 0) hsh[i] = (p < j ? 0.0 : hsh[i]) + h;  // H(i,j) (+)= h
        const double ch = mode == RES_MGS ? h : a.coef * h;
        double acc = 0.0;
        if (data) {
#pragma unroll
            for (int k = 0; k < R2; ++k) {
                wr[k].x = wr[k].x - ch * X[k].x;
                wr[k].y = wr[k].y - ch * X[k].y;
            }
            if (kind == RK_NONE) {
            } else if (last) {
#pragma unroll
                for (int k = 0; k < R2; ++k)
                    sq_acc(acc, wr[k], (c0 + k) * DT + td, tail0, mode == RES_HH_UP && c0 + k == 0);
            } else if constexpr (PF) {
#pragma unroll
                for (int k = 0; k < R2; ++k) {
                    acc = acc + wr[k].x * Y[k].x;
                    acc = acc + wr[k].y * Y[k].y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < R2; ++k)
                    if (c0 + k < cend) X[k] = ldv<NT>(colchunk(q, c0 + k) + td);
#pragma unroll
                for (int k = 0; k < R2; ++k) {
                    acc = acc + wr[k].x * X[k].x;
                    acc = acc + wr[k].y * X[k].y;
                }
            }
            const double2 *__restrict__ A2 = V2 + (i64)i * ld2;
            const double2 *__restrict__ B2 = V2 + (i64)q * ld2;
            if constexpr (L2 > 0) {  // w in LDS, its two columns stream: 16 B/unknown
                for (int k = 0; k < L2; k += 2) {
                    double2 wv[2], av[2], bv[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const i64 c = l0 + k + u;
                        if (k + u < L2 && c < lend) {
                            wv[u] = lw[(k + u) * DT + td];
                            av[u] = ldv<NT>(A2 + c * DT + td);
                            if (!last) bv[u] = a.qdef ? ldv<false>(B2 + c * DT + td) : ldv<NT>(B2 + c * DT + td);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const i64 c = l0 + k + u;
                        if (k + u < L2 && c < lend) {
                            wv[u].x = wv[u].x - ch * av[u].x;
                            wv[u].y = wv[u].y - ch * av[u].y;
                            lw[(k + u) * DT + td] = wv[u];
                            if (kind == RK_NONE) {
                            } else if (last) {
                                sq_acc(acc, wv[u], c * DT + td, tail0, mode == RES_HH_UP && c == 0);
                            } else {
                                acc = acc + wv[u].x * bv[u].x;
                                acc = acc + wv[u].y * bv[u].y;
                            }
                        }
                    }
                }
            }
            for (i64 e0 = sbase; e0 < n2; e0 += 2 * sstride) {  // streamed part: 32 B/unknown
                double2 wv[2], av[2], bv[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const i64 e = e0 + u * sstride;
                    if (e < n2) {
                        wv[u] = W2[e];
                        av[u] = ldv<NT>(A2 + e);
                        if (!last) bv[u] = a.qdef ? ldv<false>(B2 + e) : ldv<NT>(B2 + e);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const i64 e = e0 + u * sstride;
                    if (e < n2) {
                        wv[u].x = wv[u].x - ch * av[u].x;
                        wv[u].y = wv[u].y - ch * av[u].y;
                        W2[e] = wv[u];
                        if (kind == RK_NONE) {
                        } else if (last) {
                            sq_acc(acc, wv[u], e, tail0, mode == RES_HH_UP && 2 * a.nres2 < tail0);
                        } else {
                            acc = acc + wv[u].x * bv[u].x;
                            acc = acc + wv[u].y * bv[u].y;
                        }
                    }
                }
            }
            if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && td == 0) {  // odd-length tail element
                const i64 e = a.n - 1;
                const double x = a.w[e] - ch * a.V[(i64)i * a.ld + e];
                a.w[e] = x;
                if (kind == RK_DOT) acc = acc + x * a.V[(i64)q * a.ld + e];
                if (kind == RK_NORM && e >= tail0) acc = acc + x * x;
            }
        }
        if (kind == RK_NONE) return true;
        clk.passed(a.stamps);
        acc = wave_sum(acc);
        if ((t & 63) == 0) sm[t >> 6] = acc;
        __syncthreads();
        if constexpr (PF) {
            if (data && p + 2 < np) {  // the dot partner of projection p+1, in flight during the exchange
                const int q2 = res_col(mode, j, p + 2);
#pragma unroll
                for (int k = 0; k < R2; ++k)
                    if (c0 + k < cend) X[k] = ldv<NT>(colchunk(q2, c0 + k) + td);
            }
        }
        if (t < 64) res_exchange<RWAVES, MODE == RES_MGS, RES_POLL_SLEEP_SMALL>(a, xi, sm, bc, &okf);
        __syncthreads();
        ++xi;
        h = bc[0];
        clk.waited(a.stamps);
        return okf != 0;
    };
    if constexpr (PF) {
        for (int p = 0; p < np && ok; p += 2) {
            ok = proj(p, xa, xb);
            if (ok && p + 1 < np) ok = proj(p + 1, xb, xa);
        }
    } else {
        for (int p = 0; p < np && ok; ++p) ok = proj(p, xa, xb);
    }
    if (!ok) return;  // uniform per workgroup; *err is set
    if (mode != RES_MGS) {  // reflections: the resident part of w back to HBM
        if (data) {
#pragma unroll
            for (int k = 0; k < R2; ++k)
                if (c0 + k < cend) W2[(c0 + k) * DT + td] = wr[k];
            if constexpr (L2 > 0) {
                for (int k = 0; k < L2; ++k)
                    if (l0 + k < lend) W2[(l0 + k) * DT + td] = lw[k * DT + td];
            }
        }
        if (mode == RES_HH_UP && blockIdx.x == 0 && t == 0) a.hs[0] = h;  // ||w(j+1:n)||^2
        clk.finish(a.stamps, mode);
        return;
    }
    // h = ||w|| ; V(:,j+1) = w / h  (h == 0: zeros, as k_scale)
    const double hn = sqrt(h);
    double2 *__restrict__ O2 = reinterpret_cast<double2 *>(a.vout);
    if (data) {
#pragma unroll
        for (int k = 0; k < R2; ++k)
            if (c0 + k < cend)
                O2[(c0 + k) * DT + td] = res_unit(wr[k], hn);
        if constexpr (L2 > 0) {
            for (int k = 0; k < L2; ++k)
                if (l0 + k < lend) {
                    const double2 v = lw[k * DT + td];
                    O2[(l0 + k) * DT + td] = res_unit(v, hn);
                }
        }
        for (i64 e = sbase; e < n2; e += sstride) {
            const double2 v = W2[e];
            O2[e] = res_unit(v, hn);
        }
        if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && td == 0) a.vout[a.n - 1] = res_unit(a.w + a.n - 1, hn);
    }
    clk.finish(a.stamps, mode);
    res_store_hcol<RT>(a, hsh, j, hn);
}

// --------------------------------------------------------------------------
// Resident MGS-R step, w-only variant for large slabs: ONE wave per SIMD
// (256-thread workgroups, one per CU) so each lane can hold ~400 registers
// (VGPRs + AGPRs of the unified file), and they hold w only -- RW double2 per
// thread in registers and LW more in LDS.  Per projection a resident unknown
// moves 16 B (its two Krylov columns) instead of 32; the running column V_q is
// loaded with the default policy, so it is still in the Infinity Cache when
// it is read again as V_i by the next projection (V_i itself non-temporal).
// Same exchange, same arithmetic as k_mgs_res.
// PIPE (MGS step, full workgroups only -- every one holds exactly RW + LW chunks, nothing
// streamed; chosen by launch_wres): the pass keeps 14-16 column loads in flight through a
// ring of WBT buffer pairs with counted waits instead of draining each batch of 16
// (4096^2: pass 32.65 -> 31.16 us per projection, 251.8 -> 261.8 it/s).
// CARRY (> 0: the pipelined pass on a single rank, chosen by launch_wres): the ring lives at
// kernel scope and the two loads of chunks 0 .. CARRY-1 of pass p + 1 -- their addresses do
// not depend on the dot being gathered -- go out inside pass p's all-gather (head()): wave 0
// right after it has published the workgroup's granule, waves 1..3 after the barrier and
// ahead of their touches, which start CARRY chunks later (those chunks go straight to
// registers).  Pass 0's head goes out before the projection loop; after the last pass the
// head is issued on clamped columns and retired unused (no branch around a load).  The
// wait that closes every all-gather drains the head with the touches, so the pass issues
// chunks CARRY .. WBT-1 at entry and its counted waits hold unchanged; arithmetic and order
// are the pipelined pass's, results bit-identical.  Not on N ranks: there the rank-total
// pushers drain vmcnt before they publish, which would put the carried loads on every
// rank's critical path -- those launches keep CARRY = 0.  The ring registers are live
// across res_exchange and the loop back-edge: tools/asm_inflight_audit.py checks in the
// compiler's assembly that nothing names one between its load and the wait.
// --------------------------------------------------------------------------
constexpr int WT = 256;  // threads per workgroup (4 waves, one per SIMD)
#ifndef GK_RES_WB
#define GK_RES_WB 8
#endif
constexpr int WB = GK_RES_WB;        // double2 per column per batch in flight per thread
#ifndef GK_RES_WB_HH
#define GK_RES_WB_HH 6
#endif
constexpr int WB_HH = GK_RES_WB_HH;  // the reflection chains' batch (their RW is larger)
// (Round 5 removed measured-slower A/B paths from this kernel: XPF -- the next
// pass's first batch loaded before the exchange wait, 42.4 -> 46.9 us per projection
// at RW 80; ROT -- every workgroup's chunk range moved to its neighbour's, the even
// XCDs lagged as before (profiles/r02/res_trace_rotation.jsonl); REV -- the LDS part
// walked in alternating halves, 40.89 -> 44.05 us (profiles/r04/ab_rev_wb_r04i.jsonl);
// STEN -- the stencil formed in the prologue, 245.9 -> 236.2 it/s
// (profiles/r03/ab_res_sten_r03k.jsonl).  DESIGN.md 3.1 keeps the numbers.)
// TOUCH: while wave 0 runs a pass's all-gather, waves 1..3 pull the first
// TOUCH chunks (4 KiB each) of the NEXT pass's dot column -- the one that
// comes from HBM -- into L2 with one dword load per 128-B line into a sink
// register, so the memory pipe works through the wait.  0 = off; A/B at
// 4096^2 with one granule array (profiles/r02/ab_touch*.jsonl): 8 +-0, 16 -1.5 %,
// 32 -2.2 % per projection (MGS-R 42.4 -> 41.7 us, HH 43.2 -> 42.2 us), 48 / 64
// slower (the touched lines outgrow the 128 KiB per-CU share of L2); the depths
// now in use are below.
#ifndef GK_RES_TOUCH
#define GK_RES_TOUCH 24
#endif
constexpr int TOUCH = GK_RES_TOUCH;
#ifndef GK_RES_TOUCH_MGS
#define GK_RES_TOUCH_MGS 28
#endif
// Touched chunks per workgroup: MGS-R launches (paced touches) TOUCH_MGS, the
// reflection chains (burst) TOUCH.  A/B at 4096^2 after the granule replicas and the
// pacing (profiles/r02/ab_touch_depth_paced.jsonl, ab_touch_depth_mode.jsonl): MGS-R
// 16 / 20 / 24 / 28 / 32 / 40 / 48 -> 41.47 / 41.08 / 41.04 / 40.78 / 41.17 / 42.7 / 43.6
// us per projection (two boxes); Householder 24 vs 32: 40.76 vs 41.96 us per reflection.
constexpr int TOUCH_MGS = GK_RES_TOUCH_MGS;
// ... and of the MGS-R launches that run the software-pipelined pass (PIPE, below): its
// shorter pass leaves the touched lines less time in L2 and the paced touch less of a wait
// to fill.  A/B at 4096^2 on the pipelined build, three interleaved runs each
// (profiles/r07/ab_pipe_touch_r07.jsonl): 8 / 12 / 16 / 20 / 28 / 36 -> 263.3 / 264.0 /
// 264.6 / 264.8 / 258.4 / 247.2 it/s (36 on another box, where 28 gave 257.2).
#ifndef GK_RES_TOUCH_MGS_PIPE
#define GK_RES_TOUCH_MGS_PIPE 20
#endif
constexpr int TOUCH_MGS_PIPE = GK_RES_TOUCH_MGS_PIPE;
// The dot column V_q of a pass is read with the default policy, so it is still in the
// Infinity Cache when the next pass reads it as its AXPY column V_i; non-temporal like
// V_i (every column from HBM) measured 45.06 vs 41.07 us per projection.
#ifndef GK_RES_TOUCH_PACE
#define GK_RES_TOUCH_PACE 24
#endif
// TOUCH_PACE > 0 (MGS-R step launches): the touch loads go out one per lane per
// round, s_sleep TOUCH_PACE between rounds, and stop once wave 0 holds the
// exchange's total -- a late workgroup (short wait) then has few touches left to
// drain before its next pass (the trace: a workgroup late at exchange p ran its
// next pass 0.5 us longer).  A/B at 4096^2 (profiles/r02/ab_touch_pace.jsonl):
// MGS-R 41.55 -> 41.28 us per projection at 24 (8: 41.37); the reflection chains
// run slower with it (pace 8: 41.9 -> 42.7 us), so they keep the all-at-once touch.
// 0: all issued at once (drained after the exchange).  Interleaving the resident
// chunks over the grid (chunk b + kG instead of a contiguous range per workgroup)
// was measured too: 41.5 -> 48.0 us (DRAM row locality lost).
constexpr int TOUCH_PACE = GK_RES_TOUCH_PACE;
#ifndef GK_RES_TOUCH_PACE_HH
#define GK_RES_TOUCH_PACE_HH 0
#endif
// the reflection chains' pacing (0 = burst); re-measured after the depth / residency
// re-tune (profiles/r02/ab_pace_retune.jsonl): 8 / 24 -> 41.06 / 41.1 vs 40.57 us burst
constexpr int TOUCH_PACE_HH = GK_RES_TOUCH_PACE_HH;
// Ring depth of the MGS step's software-pipelined pass (k_mgs_wres<.., PIPE>, below): chunks
// whose two column loads are in flight.  10 still builds without scratch (244 AGPRs), 12
// does not; A/B at 4096^2 (profiles/r07/ab_pipe_touch_r07.jsonl): 8 vs 10 -> 258.4 vs 260.7
// it/s at touch depth 28, 264.8 vs 265.7 at 20 (samples overlap), so the ring stays at 8.
#ifndef GK_RES_PIPE_D
#define GK_RES_PIPE_D 8
#endif
constexpr int PIPE_D = GK_RES_PIPE_D;
// Chunks of the pipelined pass's ring carried across the all-gather (k_mgs_wres<.., PIPE, CARRY>):
// the first PIPE_CARRY chunk pairs of pass p + 1 are loaded inside pass p's all-gather, into
// ring registers that are otherwise empty for the whole wait.  0 = no such instantiation.
// 7 builds with 256 VGPRs + 256 AGPRs and no scratch, 8 spills.  A/B at 4096^2, builds
// interleaved on one box, three runs each (profiles/r08/ab_carry_r08.jsonl): parent / 4 / 5 / 6
// -> 259.4-260.0 / 264.9-265.6 / 265.8-267.8 / 267.5-268.7 it/s, on another box parent / 6 / 7 ->
// 262.9-263.4 / 271.9-273.2 / 273.5-275.1; pass 31.1 -> 29.3 us and wait 7.2 -> 7.45 us per
// projection at 7.  The same build with GK_TUNE_RES_PIPE_CARRY 0: 263.4.
#ifndef GK_RES_PIPE_CARRY
#define GK_RES_PIPE_CARRY 7
#endif
constexpr int PIPE_CARRY = GK_RES_PIPE_CARRY;
static_assert(PIPE_CARRY >= 0 && PIPE_CARRY <= PIPE_D, "GK_RES_PIPE_CARRY: 0 .. GK_RES_PIPE_D chunks of the ring");
// ... and the touch depth of those launches (the touches start at the first chunk that is
// not carried): 12 / 16 / 20 / 24 with 6 chunks carried -> 266.6-267.3 / 267.1-269.0 /
// 267.5-268.7 / 267.0-268.7 it/s (same file; 24 lengthens the wait 7.85 -> 8.44 us)
#ifndef GK_RES_TOUCH_MGS_CARRY
#define GK_RES_TOUCH_MGS_CARRY 20
#endif
constexpr int TOUCH_MGS_CARRY = GK_RES_TOUCH_MGS_CARRY;

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) in order: a loop
// unrolled by construction, its index a constant in the body
template <class F, int... I>
__device__ __forceinline__ void seq_apply(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void seq_for(F &&f) {
    seq_apply(f, std::make_integer_sequence<int, N>{});
}

template <int RW, int LW, int MODE, int WBT = WB, bool PIPE = false, int CARRY = 0>
__global__ __launch_bounds__(WT, 1) void k_mgs_wres(ResArgs a) {
    static_assert(CARRY >= 0 && CARRY <= WBT && (CARRY == 0 || (PIPE && MODE == RES_MGS && CARRY <= RW)),
                  "carried chunks: a head of the pipelined pass's ring, register chunks of the MGS step");
    extern __shared__ double2 lw[];  // [LW][WT]
    __shared__ double sm[WT / 64];
    __shared__ double bc[1];
    __shared__ int okf;
    __shared__ int xdone;  // PACE: the exchange in progress has completed
    // H(1:j, j): WO_HMAX entries, not RHMAX + 1 -- the MGS step's 39 LDS chunks of w leave
    // 4,048 bytes of the CU's 160 KiB (res_plan keeps m + 1 <= WO_HMAX on this kernel)
    __shared__ double hsh[MODE == RES_MGS ? WO_HMAX : 1];
    const int t = threadIdx.x;
    constexpr int mode = MODE;
    constexpr int PACE = MODE == RES_MGS ? TOUCH_PACE : TOUCH_PACE_HH;
    // touched chunks per workgroup
    constexpr int TCH = MODE == RES_MGS ? (PIPE ? (CARRY > 0 ? TOUCH_MGS_CARRY : TOUCH_MGS_PIPE) : TOUCH_MGS) : TOUCH;
    const int j = a.j, np = res_np(mode, j);
    const i64 n2 = a.n >> 1, ld2 = a.ld >> 1;
    const i64 nch = a.nres2 / WT;
    const i64 bq = blockIdx.x;  // chunk range of this workgroup
    const i64 c0 = bq * a.r2e, cend = c0 + a.r2e < nch ? c0 + a.r2e : nch;
    const i64 l0 = (i64)gridDim.x * a.r2e + bq * a.l2e, lend = l0 + a.l2e < nch ? l0 + a.l2e : nch;
    const i64 tail0 = mode == RES_HH_UP ? a.tail0 : 0;
    const double2 *__restrict__ V2 = reinterpret_cast<const double2 *>(a.V);
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(a.w);
    ResClock clk;
    clk.start(a.stamps);
    int touch_sink = 0;
    const i64 sstride = (i64)gridDim.x * WT;
    const i64 sbase = a.nres2 + (i64)res_stream_wg() * WT + t;
    double2 wr[RW];
    // CARRY: the pipelined pass's ring lives here, not in the pass: slots 0 .. CARRY-1 are
    // loaded outside it (head, below) and stay in flight across the all-gather
    [[maybe_unused]] d2v ra[CARRY > 0 ? WBT : 1], rb[CARRY > 0 ? WBT : 1];
    if (mode == RES_HH_DOWN && a.unit_init) {
        // w = e_u built in place (gmres_hh.f90:257-264): no k_set_unit launch, no read
        // of w; the streamed part is written by the thread that streams it later
        const i64 u = a.unit_e;  // local index of the 1.0, -1 on other ranks
        auto unit2 = [&](i64 e2) { return double2{2 * e2 == u ? 1.0 : 0.0, 2 * e2 + 1 == u ? 1.0 : 0.0}; };
#pragma unroll
        for (int k = 0; k < RW; ++k) wr[k] = (c0 + k < cend) ? unit2((c0 + k) * WT + t) : double2{0.0, 0.0};
        for (int k = 0; k < LW; ++k)
            if (l0 + k < lend) lw[k * WT + t] = unit2((l0 + k) * WT + t);
        for (i64 e = sbase; e < n2; e += sstride) W2[e] = unit2(e);
        if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) a.w[a.n - 1] = (a.n - 1 == u) ? 1.0 : 0.0;
    } else {
#pragma unroll
        for (int k = 0; k < RW; ++k) wr[k] = (PIPE || c0 + k < cend) ? W2[(c0 + k) * WT + t] : double2{0.0, 0.0};
        for (int k = 0; k < LW; ++k)
            if (PIPE || l0 + k < lend) lw[k * WT + t] = W2[(l0 + k) * WT + t];
    }
    // acc += the closing reduction of element pair e2 (local double2 index)
    auto red = [&](double &acc, const double2 &v, const double2 &b, int kind, i64 e2, bool chk) {
        if (kind == RK_DOT) {
            acc = acc + v.x * b.x;
            acc = acc + v.y * b.y;
        } else if (kind == RK_NORM) {
            sq_acc(acc, v, e2, tail0, chk);
        }
    };
    // One pass over the slab: w -= ch V_i, then the reduction `kind`
    // (<w, V_q>, ||w(tail0:)||^2, or none).  Returns this thread's partial.
    const i64 wc0 = c0, wl0 = l0;  // (a pass works on copies of its own)
    auto pass = [&](double ch, int i, int q, int kind) -> double {
        const double2 *__restrict__ A2 = V2 + (i64)i * ld2;
        const double2 *__restrict__ B2 = V2 + (i64)q * ld2;
        const bool dot = kind == RK_DOT;
        double acc = 0.0;
        // (pipelined instantiation: the chunk origins opaque per pass, so that the chunk
        // addresses are formed where they are used and not kept in registers across the passes)
        i64 c0 = wc0, l0 = wl0;
        if constexpr (PIPE) {
            int zero = 0;
            asm volatile("" : "+s"(zero));
            c0 += zero;
            l0 += zero;
        }
        if constexpr (PIPE) {
            // Software-pipelined pass (every workgroup holds exactly RW + LW chunks, nothing
            // streamed, n even: launch_wres).  The RW + LW chunks are walked in the same
            // order -- registers, then LDS -- through a ring of D = WBT buffer pairs (the
            // registers of the batch pass's av[] and bv[]): chunk k's two loads go into slot
            // k mod D as soon as chunk k - D is consumed, so 2 (D - 1) to 2 D loads stay in
            // flight through the whole pass.  The loads are asm statements, which the compiler
            // does not count; every chunk issues exactly two (without a dot column the second
            // one re-reads one resident chunk), loads return in issue order, so the counted
            // wait before chunk k -- two for each younger chunk in flight -- retires exactly
            // that chunk's pair.  The wait names the two buffers "+v": their arithmetic cannot
            // be scheduled above it.  Loads and waits are unconditional, straight-line code: a
            // branch around one would merge buffer values, and the compiler may place such a
            // merge's copies ahead of the wait.
            constexpr int D = WBT, NCH = RW + LW;
            static_assert(MODE == RES_MGS && NCH > D && 2 * (D - 1) <= 63,
                          "pipelined pass: the MGS step, counts within vmcnt's 6 bits, V_q default policy");
            [[maybe_unused]] d2v pl[CARRY > 0 ? 1 : D], ql[CARRY > 0 ? 1 : D];
            auto &pa = *[&]() {
                if constexpr (CARRY > 0) return &ra; else return &pl;
            }();
            auto &pb = *[&]() {
                if constexpr (CARRY > 0) return &rb; else return &ql;
            }();
            const unsigned lo = (unsigned)t * (unsigned)sizeof(double2);
            // the columns at the workgroup's register and LDS chunk ranges
            const double2 *Ar = A2 + c0 * WT, *Al = A2 + l0 * WT, *Br = B2 + c0 * WT, *Bl = B2 + l0 * WT;
            // nothing of the compiler's own is in flight from here on (it then adds no waits of
            // its own inside the pass, which would drain the loads in flight)
            __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
            // always true here, and only around a chunk's arithmetic: the test puts every
            // chunk's arithmetic in a block of its own, which is what holds the unrolled pass
            // inside the register budget
            auto held = [&](int k) { return k < RW ? c0 + k < cend : l0 + (k - RW) < lend; };
            auto issue = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                // wave-uniform chunk bases
                const double2 *ap = k < RW ? Ar + k * WT : Al + (k - RW) * WT;
                const double2 *bq = k < RW ? Br + k * WT : Bl + (k - RW) * WT;
                const double2 *bp = dot ? bq : Ar;
                d2v &da = pa[k % D], &db = pb[k % D];
                const unsigned off = lo;  // (named outside the asm operands: captured by the generic lambda)
                asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(da) : "v"(off), "s"(ap));
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(db) : "v"(off), "s"(bp));
            };
            auto wait = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int younger = NCH - 1 - k < D - 1 ? NCH - 1 - k : D - 1;  // chunks in flight behind k
                d2v &da = pa[k % D], &db = pb[k % D];
                asm volatile("s_waitcnt vmcnt(%2)" : "+v"(da), "+v"(db) : "i"(2 * younger));
            };
            auto consume = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                const double2 av{pa[k % D].x, pa[k % D].y}, bv{pb[k % D].x, pb[k % D].y};
                if (!held(k)) return;
                if constexpr (k < RW) {
                    wr[k].x = wr[k].x - ch * av.x;
                    wr[k].y = wr[k].y - ch * av.y;
                    red(acc, wr[k], bv, kind, (c0 + k) * WT + t, false);
                } else {
                    constexpr int kl = k - RW;
                    double2 wv = lw[kl * WT + t];
                    wv.x = wv.x - ch * av.x;
                    wv.y = wv.y - ch * av.y;
                    lw[kl * WT + t] = wv;
                    red(acc, wv, bv, kind, (l0 + kl) * WT + t, false);
                }
            };
            // (CARRY: chunks 0 .. CARRY-1 were issued by head() and have landed -- the wait that
            // closes every all-gather drains them -- so the counted waits below hold as they are)
            seq_for<D - CARRY>([&](auto kc) { issue(std::integral_constant<int, decltype(kc)::value + CARRY>{}); });
            seq_for<NCH>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                wait(kc);
                consume(kc);
                if constexpr (k + D < NCH) issue(std::integral_constant<int, k + D>{});
            });
            return acc;
        }
        // registers: batches of WBT chunks, both columns in flight (k0 a constant once unrolled)
        auto rbatch = [&](const int k0) {
            double2 av[WBT], bv[WBT];
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const i64 c = c0 + k0 + u;
                if (k0 + u < RW && c < cend) {
                    av[u] = ldv<true>(A2 + c * WT + t);
                    if (dot) bv[u] = ldv<false>(B2 + c * WT + t);
                }
            }
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const int k = k0 + u;
                if (k < RW && c0 + k < cend) {
                    wr[k].x = wr[k].x - ch * av[u].x;
                    wr[k].y = wr[k].y - ch * av[u].y;
                    red(acc, wr[k], bv[u], kind, (c0 + k) * WT + t, mode == RES_HH_UP && c0 + k == 0);
                }
            }
        };
        // LDS: the same, w from / to LDS
        auto lbatch = [&](const int k0, const int kend) {
            double2 av[WBT], bv[WBT];
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const i64 c = l0 + k0 + u;
                if (k0 + u < kend && c < lend) {
                    av[u] = ldv<true>(A2 + c * WT + t);
                    if (dot) bv[u] = ldv<false>(B2 + c * WT + t);
                }
            }
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const int k = k0 + u;
                if (k < kend && l0 + k < lend) {
                    double2 wv = lw[k * WT + t];
                    wv.x = wv.x - ch * av[u].x;
                    wv.y = wv.y - ch * av[u].y;
                    lw[k * WT + t] = wv;
                    red(acc, wv, bv[u], kind, (l0 + k) * WT + t, mode == RES_HH_UP && l0 + k == 0);
                }
            }
        };
#pragma unroll
        for (int k0 = 0; k0 < RW; k0 += WBT) rbatch(k0);
        for (int k0 = 0; k0 < LW; k0 += WBT) lbatch(k0, LW);
        for (i64 e0 = sbase; e0 < n2; e0 += 2 * sstride) {  // streamed part: 32 B/unknown
            double2 wv[2], av[2], bv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    wv[u] = W2[e];
                    av[u] = ldv<true>(A2 + e);
                    if (dot) bv[u] = ldv<false>(B2 + e);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    wv[u].x = wv[u].x - ch * av[u].x;
                    wv[u].y = wv[u].y - ch * av[u].y;
                    W2[e] = wv[u];
                    red(acc, wv[u], bv[u], kind, e, mode == RES_HH_UP && 2 * a.nres2 < tail0);
                }
            }
        }
        if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) {  // odd-length tail element
            const i64 e = a.n - 1;
            const double x = a.w[e] - ch * a.V[(i64)i * a.ld + e];
            a.w[e] = x;
            if (kind == RK_DOT) acc = acc + x * a.V[(i64)q * a.ld + e];
            if (kind == RK_NORM && e >= tail0) acc = acc + x * x;
        }
        return acc;
    };
    // CARRY: the two column loads of chunks 0 .. CARRY-1 of pass pn into ring slots 0 .. CARRY-1,
    // the pass's own statements (V_i non-temporal, V_q default policy, or the re-read of V_i's
    // first chunk where the pass closes with the norm).  pn = np (after the last pass): the
    // clamped columns of pass np - 1, valid addresses, retired unused -- no branch around a load.
    [[maybe_unused]] auto head = [&](int pn) {
        int zero = 0;  // (the chunk origin opaque per issue site, as in a pass)
        asm volatile("" : "+s"(zero));
        const double2 *Ar = V2 + (i64)res_col(mode, j, pn) * ld2 + (wc0 + zero) * WT;
        const double2 *Br = V2 + (i64)res_col(mode, j, pn + 1) * ld2 + (wc0 + zero) * WT;
        const bool dot = pn < np - 1;
        const unsigned lo = (unsigned)t * (unsigned)sizeof(double2);
        seq_for<CARRY>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const double2 *ap = Ar + k * WT;
            const double2 *bp = dot ? Br + k * WT : Ar;
            d2v &da = ra[k], &db = rb[k];
            const unsigned off = lo;  // (named outside the asm operands: captured by the generic lambda)
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(da) : "v"(off), "s"(ap));
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(db) : "v"(off), "s"(bp));
        });
    };
    // ... and the point from which the carried slots hold their data: everything in flight
    // has landed, and nothing that reads a slot can be placed above it
    [[maybe_unused]] auto head_landed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        seq_for<CARRY>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            d2v &da = ra[k], &db = rb[k];
            asm volatile("" : "+v"(da), "+v"(db));
        });
    };
    // all-gather of the partials: the same h in every workgroup (and rank)
    // (CARRY: pass head_p's first chunks go out inside it -- wave 0 once its granule is
    // published, waves 1..3 ahead of their touches, which then start CARRY chunks later)
    int xi = 0;
    auto reduce = [&](double acc, double &h, int touch_col, [[maybe_unused]] int head_p = 0) -> bool {
        clk.passed(a.stamps);
        acc = wave_sum(acc);
        if ((t & 63) == 0) sm[t >> 6] = acc;
        if (PACE > 0 && t == 0) xdone = 0;
        __syncthreads();
        // (CARRY: each arm has its own head issue into the same ring registers.  A wave runs one
        // arm only -- t < 64 holds for whole waves -- but the compiler lays them out as two
        // masked blocks in a row; the comment each arm opens with tells
        // tools/asm_inflight_audit.py, which reads the assembly, that no wave runs both.)
        if (t < 64) {
            if constexpr (CARRY > 0) {
                asm volatile("; gk-audit: arm wave0");
                res_exchange<WT / 64, MODE == RES_MGS, RES_POLL_SLEEP>(a, xi, sm, bc, &okf, [&]() { head(head_p); });
            } else {
                res_exchange<WT / 64, MODE == RES_MGS, RES_POLL_SLEEP>(a, xi, sm, bc, &okf);
            }
            if (PACE > 0 && t == 0) *(volatile int *)&xdone = 1;
        } else {
            if constexpr (CARRY > 0) {
                asm volatile("; gk-audit: arm waves123");
                head(head_p);
            }
            if (TCH > 0 && touch_col >= 0) {
                // lines [0, 32*TCH) of the workgroup's register-resident part of
                // the column (contiguous from chunk c0, CARRY: from the first chunk that
                // is not carried); all loads land in one sink
                // register, drained below before anything can reuse it
                const i64 r0 = c0 + CARRY, r1 = cend;
                const i64 lines = (i64)32 * (r1 - r0 < TCH ? (r1 - r0 > 0 ? r1 - r0 : 0) : TCH);
                const char *base = reinterpret_cast<const char *>(V2 + (i64)touch_col * ld2 + r0 * WT);
                res_touch<PACE>(base, lines, t - 64, WT - 64, &xdone, touch_sink);
            }
        }
        __syncthreads();
        if constexpr (CARRY > 0) asm volatile("; gk-audit: arms end");
        if constexpr (TCH > 0) asm volatile("s_waitcnt vmcnt(0)" : : "v"(touch_sink) : "memory");
        if constexpr (CARRY > 0) head_landed();
        ++xi;
        h = bc[0];
        clk.waited(a.stamps);
        return okf != 0;
    };
    // The last pass of a reflection chain reduces nothing: RES_HH_UP's closing
    // ||w(j+1:n)||^2 is taken after the loop, from the registers w is written
    // back from, so the pass code of all three modes is the same (the tail test
    // inside the unrolled loop made the UP pass 28 % slower: 45.9 vs 35.7 us).
    auto kind_of = [&](int p) { return p < np - 1 ? RK_DOT : (mode == RES_MGS ? RK_NORM : RK_NONE); };
    double h;
    bool ok = true;
    if (mode == RES_HH_DOWN) {
        // the pre-dot as an AXPY pass with h = 0 (w - 0 V = w): a dot-only copy of the
        // unrolled register loop would not fit the register file
        const int q = res_col(mode, j, 0);
        double acc = 0.0;
        if (a.unit_known) {  // <e_u, P_q> = P_q(u): the one nonzero product, as the full sum gives it
            if (blockIdx.x == 0 && t == 0 && a.unit_e >= 0) acc = a.V[(i64)q * a.ld + a.unit_e];
        } else {
            acc = pass(0.0, q, q, RK_DOT);
        }
        ok = reduce(acc, h, kind_of(0) == RK_DOT ? res_col(mode, j, 1) : -1);
    } else {
        double s = 0.0;
        for (int k = t; k < a.npin; k += WT) s += a.pin[k];
        s = wave_sum(s);
        if ((t & 63) == 0) sm[t >> 6] = s;
        __syncthreads();
        h = sm[0];
#pragma unroll
        for (int w = 1; w < WT / 64; ++w) h += sm[w];
        __syncthreads();
        ok = res_pin_fold(a, h, bc, &okf);
    }
    if constexpr (CARRY > 0) {  // pass 0's head (every later one goes out in the all-gather before it)
        head(0);
        head_landed();
    }
    for (int p = 0; p < np && ok; ++p) {
        const int i = res_col(mode, j, p);
        const int kind = kind_of(p);
        if (mode == RES_MGS && blockIdx.x == 0 && t == 0) hsh[i] = (p < j ? 0.0 : hsh[i]) + h;  // H(i,j) (+)= h
        const double acc = pass(mode == RES_MGS ? h : a.coef * h, i, res_col(mode, j, p + 1), kind);
        if (kind != RK_NONE)
            ok = reduce(acc, h, p + 1 < np && kind_of(p + 1) == RK_DOT ? res_col(mode, j, p + 2) : -1, p + 1);
    }
    if (!ok) return;  // uniform per workgroup; *err is set
    const bool close = mode == RES_HH_UP && a.close_hh;
    if (mode != RES_MGS) {  // reflections: the resident part of w back to HBM (not when close)
        double acc = 0.0;  // RES_HH_UP: ||w(j+1:n)||^2, local indices >= tail0
        const bool up = mode == RES_HH_UP;
#pragma unroll
        for (int k = 0; k < RW; ++k)
            if (c0 + k < cend) {
                if (!close) W2[(c0 + k) * WT + t] = wr[k];
                if (up) sq_acc(acc, wr[k], (c0 + k) * WT + t, tail0, c0 + k == 0);
            }
        for (int k = 0; k < LW; ++k)
            if (l0 + k < lend) {
                const double2 v = lw[k * WT + t];
                if (!close) W2[(l0 + k) * WT + t] = v;
                if (up) sq_acc(acc, v, (l0 + k) * WT + t, tail0, l0 + k == 0);
            }
        if (up) {
            for (i64 e = sbase; e < n2; e += sstride) sq_acc(acc, W2[e], e, tail0, 2 * e < tail0 + 2);
            if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0 && a.n - 1 >= tail0) {
                const double x = a.w[a.n - 1];
                acc = acc + x * x;
            }
            ok = reduce(acc, h, -1);
            if (!ok) return;
            if (blockIdx.x == 0 && t == 0) a.hs[0] = h;  // ||w(j+1:n)||^2
        }
        if (!close) {
            clk.finish(a.stamps, mode);
            return;
        }
        // Next reflector in the same launch (gmres_hh.f90:306-318; k_hh_pivot + k_hh_fix +
        // k_scale of the launch path, the same element arithmetic): on the rank owning
        // w(j+1) (local index f = tail0 >= 0) H(j+1,j) = w(j+1) > 0 ? -tmp : tmp with tmp =
        // sqrt(h), w(1:j) = 0, w(j+1) = w(j+1) - H; then P(:,j+1) = w / ||w||.  w(1:j+1)
        // before the fix goes to hb for the pivot kernel (the H column).  The indices <= f
        // lie in chunks 0 and 1 (f <= RHMAX): the per-element test runs there only.
        const double s = sqrt(h);
        const i64 f = tail0;
        auto fix1 = [&](double &x, i64 g) {
            if (g < f) {
                a.hb[g] = x;
                x = 0.0;
            } else if (g == f) {
                a.hb[g] = x;
                const double dl = (x > 0.0) ? s : -s;  // delta = -H
                x = x + dl;
            }
        };
        auto fix_sq = [&](double &acc2, double2 &v, i64 e2, bool chk) {
            if (chk) {
                fix1(v.x, 2 * e2);
                fix1(v.y, 2 * e2 + 1);
            }
            acc2 = acc2 + v.x * v.x;
            acc2 = acc2 + v.y * v.y;
        };
        const i64 cfix = f >= 0 ? f / (2 * WT) : -1;  // last chunk holding an index <= f
        double acc2 = 0.0;
#pragma unroll
        for (int k = 0; k < RW; ++k)
            if (c0 + k < cend) fix_sq(acc2, wr[k], (c0 + k) * WT + t, c0 + k <= cfix);
        for (int k = 0; k < LW; ++k)
            if (l0 + k < lend) {
                double2 v = lw[k * WT + t];
                const bool chk = l0 + k <= cfix;
                fix_sq(acc2, v, (l0 + k) * WT + t, chk);
                if (chk) lw[k * WT + t] = v;
            }
        for (i64 e = sbase; e < n2; e += sstride) {
            double2 v = W2[e];
            const bool chk = 2 * e <= f;
            fix_sq(acc2, v, e, chk);
            if (chk) W2[e] = v;
        }
        if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) {
            double x = a.w[a.n - 1];
            if (a.n - 1 <= f) {
                fix1(x, a.n - 1);
                a.w[a.n - 1] = x;
            }
            acc2 = acc2 + x * x;
        }
        ok = reduce(acc2, h, -1);
        if (!ok) return;
    }
    const double hn = sqrt(h);
    double2 *__restrict__ O2 = reinterpret_cast<double2 *>(a.vout);
    if constexpr (PIPE) {  // (as in a pass: the chunk addresses formed here, not kept from the prologue)
        int zero = 0;
        asm volatile("" : "+s"(zero));
        O2 += zero;
    }
#pragma unroll
    for (int k = 0; k < RW; ++k)
        if (PIPE || c0 + k < cend)  // (the pipelined instantiation runs on full workgroups only)
            O2[(c0 + k) * WT + t] = res_unit(wr[k], hn);
    for (int k = 0; k < LW; ++k)
        if (PIPE || l0 + k < lend) {
            const double2 v = lw[k * WT + t];
            O2[(l0 + k) * WT + t] = res_unit(v, hn);
        }
    for (i64 e = sbase; e < n2; e += sstride) {
        const double2 v = W2[e];
        O2[e] = res_unit(v, hn);
    }
    if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) a.vout[a.n - 1] = res_unit(a.w + a.n - 1, hn);
    clk.finish(a.stamps, mode);
    if (mode == RES_MGS) res_store_hcol<WT>(a, hsh, j, hn);
}


// --------------------------------------------------------------------------
// Resident MGS-R step, column-cache variant (k_mgs_wres's structure, NT-thread
// workgroups, one per CU, two waves per SIMD at NT = 512 -- the second wave
// keeps a batch of loads in flight while the first consumes its own): w wholly in
// registers (RW
// double2 per thread) and the running Krylov column cached on chip -- RX
// double2 per thread in registers, LX more in LDS.  A pass reads only its dot
// column V_q (its AXPY column V_i is the previous pass's V_q, still cached):
// 8 B per unknown per projection, against 16 B for the w-only kernel and for
// k_mgs_res's LDS-held w.  For slabs of up to RW chunks per thread -- the slab
// of one GPU of 4096^2 / 2 and of 8192^2 / 8 is 64 (RX + LX = 62 cached), of
// 4096^2 / 4 is 32.  Chunks past RX + LX (not cached) read V_i too (16 B),
// chunks past RW stream (32 B).  Same exchange, same element arithmetic as
// k_mgs_res / k_mgs_wres; only the dot summation order within a thread
// differs.  Columns non-temporal (nothing is re-read through the caches).
// --------------------------------------------------------------------------
template <int RW, int RX, int LX, int MODE, int WBT = 8, int NT = WT>
__global__ __launch_bounds__(NT, 1) void k_mgs_wpc(ResArgs a) {
    static_assert(RX <= RW && RX + LX <= RW, "the column cache covers register chunks of w only");
    extern __shared__ double2 lx[];  // [LX][NT]: cached column of chunks RX .. RX + LX - 1
    __shared__ int xdone;            // the exchange in progress has completed (stops the touches)
    __shared__ double sm[NT / 64];
    __shared__ double bc[1];
    __shared__ int okf;
    __shared__ double hsh[RHMAX + 1];
    const int t = threadIdx.x;
    constexpr int mode = MODE;
    const int j = a.j, np = res_np(mode, j);
    const i64 n2 = a.n >> 1, ld2 = a.ld >> 1;
    const i64 nch = a.nres2 / NT;
    const i64 c0 = (i64)blockIdx.x * a.r2e, cend = c0 + a.r2e < nch ? c0 + a.r2e : nch;
    const i64 tail0 = mode == RES_HH_UP ? a.tail0 : 0;
    const double2 *__restrict__ V2 = reinterpret_cast<const double2 *>(a.V);
    double2 *__restrict__ W2 = reinterpret_cast<double2 *>(a.w);
    ResClock clk;
    clk.start(a.stamps);
    const i64 sstride = (i64)gridDim.x * NT;
    const i64 sbase = a.nres2 + (i64)res_stream_wg() * NT + t;
    double2 wr[RW], xc[RX > 0 ? RX : 1];
    {  // w, and the AXPY column of pass 0 into the cache
        const double2 *__restrict__ C2 = V2 + (i64)res_col(mode, j, 0) * ld2;
#pragma unroll
        for (int k = 0; k < RW; ++k) wr[k] = (c0 + k < cend) ? W2[(c0 + k) * NT + t] : double2{0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RX; ++k) xc[k] = (c0 + k < cend) ? ldv<true>(C2 + (c0 + k) * NT + t) : double2{0.0, 0.0};
        for (int k = 0; k < LX; ++k)
            if (c0 + RX + k < cend) lx[k * NT + t] = ldv<true>(C2 + (c0 + RX + k) * NT + t);
    }
    // One pass: w -= ch V_i (the cached column; V_i from HBM past the cache), then
    // the reduction `kind`; with a dot, V_q replaces the cached column.  Batches of
    // WBT chunks (A/B, profiles/r04/ab_wpc_r04d.jsonl: software-pipelining the
    // batches -- batch b + 1 issued before b is consumed -- was slower, 17.5 ->
    // 18.3 us per projection at 2896^2, and so were 4- and 16-chunk batches).
    auto pass = [&](double ch, int i, int q, int kind) -> double {
        const double2 *__restrict__ A2 = V2 + (i64)i * ld2;
        const double2 *__restrict__ B2 = V2 + (i64)q * ld2;
        const bool dot = kind == RK_DOT;
        double acc = 0.0;
#pragma unroll
        for (int k0 = 0; k0 < RW; k0 += WBT) {
            double2 av[WBT], bv[WBT];
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const int k = k0 + u;
                const i64 c = c0 + k;
                if (k < RW && c < cend) {
                    if (dot) bv[u] = ldv<true>(B2 + c * NT + t);
                    if (k >= RX + LX) av[u] = ldv<true>(A2 + c * NT + t);  // not cached
                }
            }
#pragma unroll
            for (int u = 0; u < WBT; ++u) {
                const int k = k0 + u;
                if (k < RW && c0 + k < cend) {
                    double2 x;
                    if (k < RX)
                        x = xc[k < RX ? k : 0];
                    else if (k < RX + LX)
                        x = lx[(k - RX) * NT + t];
                    else
                        x = av[u];
                    wr[k].x = wr[k].x - ch * x.x;
                    wr[k].y = wr[k].y - ch * x.y;
                    if (dot) {
                        acc = acc + wr[k].x * bv[u].x;
                        acc = acc + wr[k].y * bv[u].y;
                        if (k < RX)
                            xc[k < RX ? k : 0] = bv[u];
                        else if (k < RX + LX)
                            lx[(k - RX) * NT + t] = bv[u];
                    } else if (kind == RK_NORM) {
                        sq_acc(acc, wr[k], (c0 + k) * NT + t, tail0, mode == RES_HH_UP && c0 + k == 0);
                    }
                }
            }
        }
        for (i64 e0 = sbase; e0 < n2; e0 += 2 * sstride) {  // streamed part: 32 B/unknown
            double2 wv[2], av[2], bv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    wv[u] = W2[e];
                    av[u] = ldv<true>(A2 + e);
                    if (dot) bv[u] = ldv<true>(B2 + e);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const i64 e = e0 + u * sstride;
                if (e < n2) {
                    wv[u].x = wv[u].x - ch * av[u].x;
                    wv[u].y = wv[u].y - ch * av[u].y;
                    W2[e] = wv[u];
                    if (dot) {
                        acc = acc + wv[u].x * bv[u].x;
                        acc = acc + wv[u].y * bv[u].y;
                    } else if (kind == RK_NORM) {
                        sq_acc(acc, wv[u], e, tail0, mode == RES_HH_UP && 2 * a.nres2 < tail0);
                    }
                }
            }
        }
        if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) {  // odd-length tail element
            const i64 e = a.n - 1;
            const double x = a.w[e] - ch * a.V[(i64)i * a.ld + e];
            a.w[e] = x;
            if (dot) acc = acc + x * a.V[(i64)q * a.ld + e];
            if (kind == RK_NORM && e >= tail0) acc = acc + x * x;
        }
        return acc;
    };
    // The all-gather on wave 0.  (xdone and touch_col served a touch of the next pass's dot
    // column into L2 by the other waves meanwhile: it lengthened the wait by what it took
    // off the pass, ab_wpc_touch_r04e.  The flag's two stores stay so the kernel is the
    // one that was measured.)
    int xi = 0;
    auto reduce = [&](double acc, double &h, int touch_col) -> bool {
        clk.passed(a.stamps);
        acc = wave_sum(acc);
        if ((t & 63) == 0) sm[t >> 6] = acc;
        if (t == 0) xdone = 0;
        __syncthreads();
        if (t < 64) {
            res_exchange<NT / 64, MODE == RES_MGS, RES_POLL_SLEEP_PC>(a, xi, sm, bc, &okf);
            if (t == 0) *(volatile int *)&xdone = 1;
        }
        __syncthreads();
        ++xi;
        h = bc[0];
        clk.waited(a.stamps);
        return okf != 0;
    };
    auto kind_of = [&](int p) { return p < np - 1 ? RK_DOT : (mode == RES_HH_DOWN ? RK_NONE : RK_NORM); };
    auto next_dot_col = [&](int p) { return p + 1 < np && kind_of(p + 1) == RK_DOT ? res_col(mode, j, p + 2) : -1; };
    double h;
    bool ok = true;
    if (mode == RES_HH_DOWN) {
        // the pre-dot <v, V_col(0)> as a pass with h = 0 (w - 0 V = w; the cache is
        // refilled with the same column)
        const int q = res_col(mode, j, 0);
        double acc = 0.0;
        if (a.unit_known) {  // <e_u, P_q> = P_q(u): the one nonzero product, as the full sum gives it
            if (blockIdx.x == 0 && t == 0 && a.unit_e >= 0) acc = a.V[(i64)q * a.ld + a.unit_e];
        } else {
            acc = pass(0.0, q, q, RK_DOT);
        }
        ok = reduce(acc, h, kind_of(0) == RK_DOT ? res_col(mode, j, 1) : -1);
    } else {
        double s = 0.0;
        for (int k = t; k < a.npin; k += NT) s += a.pin[k];
        s = wave_sum(s);
        if ((t & 63) == 0) sm[t >> 6] = s;
        __syncthreads();
        h = sm[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) h += sm[w];
        __syncthreads();
        ok = res_pin_fold(a, h, bc, &okf);
    }
    for (int p = 0; p < np && ok; ++p) {
        const int i = res_col(mode, j, p);
        const int kind = kind_of(p);
        if (mode == RES_MGS && blockIdx.x == 0 && t == 0) hsh[i] = (p < j ? 0.0 : hsh[i]) + h;  // H(i,j) (+)= h
        const double acc = pass(mode == RES_MGS ? h : a.coef * h, i, res_col(mode, j, p + 1), kind);
        if (kind != RK_NONE) ok = reduce(acc, h, next_dot_col(p));
    }
    if (!ok) return;  // uniform per workgroup; *err is set
    if (mode != RES_MGS) {  // reflections: w back to HBM (RES_HH_UP: h = ||w(j+1:n)||^2)
#pragma unroll
        for (int k = 0; k < RW; ++k)
            if (c0 + k < cend) W2[(c0 + k) * NT + t] = wr[k];
        if (mode == RES_HH_UP && blockIdx.x == 0 && t == 0) a.hs[0] = h;
        clk.finish(a.stamps, mode);
        return;
    }
    const double hn = sqrt(h);
    double2 *__restrict__ O2 = reinterpret_cast<double2 *>(a.vout);
#pragma unroll
    for (int k = 0; k < RW; ++k)
        if (c0 + k < cend)
            O2[(c0 + k) * NT + t] = res_unit(wr[k], hn);
    for (i64 e = sbase; e < n2; e += sstride) {
        const double2 v = W2[e];
        O2[e] = res_unit(v, hn);
    }
    if ((a.n & 1) && blockIdx.x == gridDim.x - 1 && t == 0) a.vout[a.n - 1] = res_unit(a.w + a.n - 1, hn);
    clk.finish(a.stamps, mode);
    res_store_hcol<NT>(a, hsh, j, hn);
}


// ---------------------------------------------------------------- planner ---
constexpr int RES_LDS_MIN = 96 * 1024;  // dynamic LDS: > half a CU's 160 KiB, so one workgroup per CU
constexpr int RES_L2 = 18;              // LDS-resident double2 of w per data thread (18 x 512 x 16 B = 144 KiB)

#ifndef GK_RES_RW
#define GK_RES_RW 89
#endif
#ifndef GK_RES_LW
#define GK_RES_LW 39
#endif
// w-only variant: double2 of w per thread in registers / LDS.  The MGS step holds 89 + 39
// chunks -- the whole 4096^2 slab on chip, nothing streamed -- since round 5 sized its H
// column in LDS by m (gk::WO_HMAX) instead of RHMAX; rounds 1-4 held 88 + 38 and streamed
// 1.5 % of w at 32 B per unknown.  The reflection chains keep 90 + 38 (RES_RW_HH, RES_LW_HH).
constexpr int RES_RW = GK_RES_RW, RES_LW = GK_RES_LW, RES_LW_HH = 38;
#ifndef GK_RES_RW_HH
#define GK_RES_RW_HH 90
#endif
// The reflection chains hold two chunks more (RW 90 with a 6-deep batch: 90 + 38 chunks =
// the whole 4096^2 slab on chip, nothing streamed): A/B at 4096^2 (profiles/r02/ab_rw_hh.jsonl)
// Householder 41.05 -> 40.57 us per reflection, while the MGS-R step keeps 88 / 8 (41.2 vs
// 41.67 us with 90 / 6).
constexpr int RES_RW_HH = GK_RES_RW_HH;
#ifndef GK_RES_PIPE
#define GK_RES_PIPE 1
#endif
// The w-only MGS step's software-pipelined pass (k_mgs_wres<.., PIPE = true>: the column
// loads of half-batch b + 1 in flight while half-batch b is consumed, counted waits), the
// default of GK_TUNE_RES_PIPE.  It runs only where every workgroup holds exactly RES_RW +
// RES_LW chunks and nothing is streamed (4096^2 on 256 CUs); every other plan runs the
// batch-by-batch pass.  A/B at 4096^2, parent build and this one interleaved on one box, three
// runs each (profiles/r07/ab_pipe_touch_r07.jsonl): 251.5 / 251.8 / 251.9 -> 261.8 / 262.0 /
// 261.8 it/s, pass 32.65 -> 31.16 us and wait 7.53 -> 7.23 us per projection (with the touch
// depth of these launches re-tuned 28 -> 20; at 28: 250.9-252.1 -> 257.0-257.5 it/s); the
// same build with GK_TUNE_RES_PIPE 0: 251.8.  Results bit-identical to the batch pass.
constexpr bool RES_PIPE = GK_RES_PIPE != 0;
// (what the pipelined pass asserts: its wait counts within vmcnt's 6 bits, V_q default policy)
constexpr bool RES_PIPE_OK = 2 * (gk::PIPE_D - 1) <= 63 && RES_RW + RES_LW > gk::PIPE_D;

// Column-cache variant (k_mgs_wpc): w of up to RES_PC_RW chunks per thread in
// registers, the running column of RES_PC_RX of them in registers and of
// RES_PC_LX in LDS; a pass streams its dot column in batches of WB chunks.
// Workgroups of 512 threads, two waves per SIMD (one wave's batch is in flight while
// the other consumes its own): 32 chunks of w per thread, 4 + 19 of the column cached
// (the 9 others read V_i too: 10.25 B per unknown at 2896^2), batches of 4 -- 13 + 19
// cached spill at 256 VGPRs per wave (the two-wave budget).  The first build, one wave
// per SIMD with 64 chunks per thread, ran 17.6 us per projection at 2896^2 against 15.5
// (profiles/r04/ab_pc512_r04j.jsonl) and is gone; so is its touch of the next pass's dot
// column into L2 during each all-gather (touch 28 / 16 / 0 -> 18.2 / 17.8 / 17.6 us per
// projection, ab_wpc_touch_r04e).
#ifndef GK_RES_PC_WB
#define GK_RES_PC_WB 4
#endif
#ifndef GK_RES_PC_WB_HH
#define GK_RES_PC_WB_HH 4
#endif
#ifndef GK_RES_PC_RX
#define GK_RES_PC_RX 4
#endif
constexpr int RES_PC_NT = 512;
#ifndef GK_RES_PC_RX_MGS
#define GK_RES_PC_RX_MGS 6
#endif
// RX_MGS: the MGS step's register-cached chunks (6 fit its register budget; the
// reflection chains spill 20 B per lane at 6 and keep RX = 4)
constexpr int RES_PC_RW = 32, RES_PC_RX = GK_RES_PC_RX, RES_PC_LX = 19;
constexpr int RES_PC_RX_MGS = GK_RES_PC_RX_MGS;
constexpr int RES_PC_WB = GK_RES_PC_WB, RES_PC_WB_HH = GK_RES_PC_WB_HH;
// Slabs of at most 16 chunks per thread: k_mgs_wpc<16, 16, 0> -- w and
// its whole column in registers, no LDS, half the unrolled pass of the 32-chunk kernel.
#ifndef GK_RES_PC_SMALL
#define GK_RES_PC_SMALL 1
#endif
constexpr bool RES_PCS = GK_RES_PC_SMALL != 0;
constexpr int RES_PCS_RW = 16, RES_PCS_RX = 16, RES_PCS_LX = 0;

// Modelled bytes per projection of a slab of n2 double2 on G workgroups (the
// unit of pairs_bytes / wonly_bytes: 8 per double2 whose w and running column are
// on chip, 16 per double2 of w alone, 32 per streamed double2) under the
// column-cache variant: the cached pairs, the rest of the register-held w, the
// streamed rest.
i64 pc_bytes(i64 n2, int G, bool hh) {
    if (RES_PCS && n2 <= (i64)G * RES_PCS_RW * RES_PC_NT) return 8 * n2;  // the 16-chunk kernel: all cached
    const int rx = hh ? RES_PC_RX : RES_PC_RX_MGS;
    const i64 cap = (i64)G * RES_PC_RW * RES_PC_NT, cached = (i64)G * (rx + RES_PC_LX) * RES_PC_NT;
    const i64 r = std::min(n2, cap), c = std::min(r, cached);
    return 8 * c + 16 * (r - c) + 32 * (n2 - r);
}

// Modelled fabric bytes per projection (per double2) of the two large-slab
// variants: pairs (w + running column, 8 B/unknown) in 2 x 12 registers + w in
// LDS (16 B) vs w only in registers + LDS (16 B); the rest streams (32 B).
i64 pairs_bytes(i64 n2, int G) {  // k_mgs_res<12, 18>: 2 x 12 registers + 18 LDS chunks of w
    const i64 rp = (i64)G * RES_R2_BIG * gk::RT, lp = (i64)G * RES_L2 * gk::RT;
    auto clamp = [](i64 v) { return v < 0 ? (i64)0 : v; };
    const i64 pr = std::min(n2, rp), pl = std::min(clamp(n2 - rp), lp), ps = clamp(n2 - rp - lp);
    return 8 * pr + 16 * pl + 32 * ps;
}

i64 wonly_bytes(i64 n2, int G) {
    const i64 rw = (i64)G * (RES_RW + RES_LW) * gk::WT;  // (the MGS step's; the reflection chains' is the same 128)
    const i64 wr = std::min(n2, rw), ws = n2 > rw ? n2 - rw : 0;
    return 16 * wr + 32 * ws;
}

static bool wonly_pays(i64 n2, int G) { return wonly_bytes(n2, G) < pairs_bytes(n2, G); }

void res_spread(i64 n2, i64 dt, int G, int rmax, int lmax, int &r2e, int &l2e, i64 &nres2) {
    const i64 nchf = n2 / dt;
    r2e = (int)std::min<i64>(rmax, (nchf + G - 1) / G);
    const i64 rest = std::max<i64>(0, nchf - (i64)G * r2e);
    l2e = (int)std::min<i64>(lmax, (rest + G - 1) / G);
    nres2 = std::min<i64>(nchf, (i64)G * (r2e + l2e)) * dt;
}

// The variant a slab of nloc local unknowns runs on (pure: no context, no
// device; gk_res_plan_query exposes it so the CPU tests pin what every
// production split selects).
//   fits in 3 x R2 <= 8 registers (w, running column, prefetched column) with
//   wave 0 kept for the exchange: R2 in {2,4,8}, PF + CW;
//   else w only in registers + LDS when the byte model says so (GK_TUNE_RES_WONLY);
//   else w and the running column in 2 x 12 registers, plus
//   w of 18 more chunks per workgroup in LDS, the rest streamed.
void plan_resident(i64 nloc, int gmax, int cap, int tune_wonly, bool hh, bool nt, ResPlan &p,
                   int tune_pc, int tune_blk, int tune_pf, int tune_pipe, int tune_carry) {
    const i64 n2 = nloc / 2;
    const i64 dcw = gk::RT - 64;
    // small vectors: no more workgroups than two chunks each (a cheaper all-gather)
    const int gcw = (int)std::max<i64>(1, std::min<i64>(gmax, (n2 + 2 * dcw - 1) / (2 * dcw)));
    const i64 need = (n2 + (i64)gcw * dcw - 1) / ((i64)gcw * dcw);
    p = ResPlan{};
    static const int pfs[] = {2, 4, 8};
    for (int s : pfs)
        if (s <= cap && (p.r2 == 0 || p.r2 < need)) p.r2 = s;
    // the resident chunks spread evenly over the p.G workgroups chosen below
    auto spread = [&](i64 dt, int rmax, int lmax) { res_spread(n2, dt, p.G, rmax, lmax, p.r2e, p.l2e, p.nres2); };
    // The column-cache variant where it moves fewer bytes than both large-slab
    // variants: it streams as fast as k_mgs_res (2896^2: 10.25 vs 14 B/unknown -> 15.5
    // vs 18.8 us per projection; 2048^2: 8 vs 10 -> 8.8 vs 9.6,
    // profiles/r04/ab_pc512_r04j.jsonl).
    const int var = gk::blk_variant((n2 + (i64)gmax * 512 - 1) / ((i64)gmax * 512));
    // The strict step on k_mgs_blk<S = 1> (the next dot column prefetched into LDS during each
    // all-gather), opt-in (GK_TUNE_RES_PF 1) for slabs up to 32 chunks of 512.  Faster than the
    // strict kernels only at 16 chunks on one GPU (2048^2 8.04 -> 7.64 us per projection;
    // 1024^2 3.78 -> 4.33, 1448^2 5.67 -> 5.77, 2896^2 15.0 -> 20.5: profiles/r05/
    // ab_strict_pf_r05w.txt), and at the load it helps -- the 4096^2 / 4 split -- the 4-rank
    // same-device rehearsal ran slower on it (1,061 vs 1,110 it/s, its all-gather wait 3.9 ->
    // 7.6 us: reh4_2048_pf_r05x.json vs reh4_2048_r05z.json), so it is not the default.
    const bool pf = !hh && tune_blk == 1 && var != gk::BLK_WONLY && tune_pf > 0;
    if (!hh && (tune_blk > 1 || pf)) {
        // the blocked-projection MGS step (opt-in): the instantiation by the chunks of
        // 512 double2 a workgroup holds -- w in registers (+ LDS for the w-only build)
        // and blocks of S columns cached where they fit (gk_blk.hpp); S = 1
        // (GK_TUNE_RES_PF): the strict step on the same kernel and its LDS prefetch
        p.G = gmax;
        const gk::BlkGeom g = gk::blk_geom(var, tune_blk);
        p.blk = tune_blk;
        p.bvar = var;
        p.wt = g.nt;
        spread(g.nt, g.rw, g.lw);
        p.r2 = g.rx;
        p.l2 = g.lx;
        p.lds = (g.lw + tune_blk * (g.lx + g.pfx)) * g.nt * (int)sizeof(double2);
        p.nt = true;
        return;
    }
    const bool pc_fits = n2 <= (i64)gmax * RES_PC_RW * RES_PC_NT;
    const i64 other_bytes = std::min(pairs_bytes(n2, gmax), wonly_bytes(n2, gmax));
    const bool pc_pays = pc_fits && pc_bytes(n2, gmax, hh) < other_bytes;
    if (p.r2 >= need || cap < RES_R2_BIG) {
        p.G = gcw;
        p.pf = p.cw = true;
        spread(dcw, p.r2, 0);
    } else if (tune_wonly <= 0 && (tune_pc > 0 ? pc_fits : (tune_pc < 0 && pc_pays))) {
        // w wholly in registers, the running column cached (k_mgs_wpc): 8 B/unknown
        p.G = gmax;
        p.pc = true;
        p.wt = RES_PC_NT;
        spread(RES_PC_NT, RES_PC_RW, 0);
        p.pcs = RES_PCS && p.r2e <= RES_PCS_RW;
        p.r2 = p.pcs ? RES_PCS_RX : (hh ? RES_PC_RX : RES_PC_RX_MGS);
        p.l2 = p.pcs ? RES_PCS_LX : RES_PC_LX;
        p.lds = p.l2 * RES_PC_NT * (int)sizeof(double2);
        p.nt = true;
        return;
    } else if (tune_wonly > 0 || (tune_wonly < 0 && wonly_pays(n2, gmax))) {
        // w only, one wave per SIMD: 16 B/unknown per projection for ~100 chunks per workgroup
        p.G = gmax;
        p.wo = true;
        p.wt = gk::WT;
        p.r2 = 0;  // (the kernel's register part is RES_RW / RES_RW_HH chunks: r2e)
        spread(gk::WT, hh ? RES_RW_HH : RES_RW, hh ? RES_LW_HH : RES_LW);
        p.lds = (hh ? RES_LW_HH : RES_LW) * gk::WT * (int)sizeof(double2);
        p.nt = true;  // V_i non-temporal, V_q default policy (fixed in the kernel)
        // The pipelined pass counts its loads: only where every workgroup holds exactly
        // RES_RW + RES_LW whole chunks, nothing is streamed and there is no odd element.
        p.pipe = RES_PIPE_OK && !hh && (tune_pipe < 0 ? RES_PIPE : tune_pipe != 0) && p.r2e == RES_RW &&
                 p.l2e == RES_LW && nloc % 2 == 0 && n2 == (i64)p.G * (RES_RW + RES_LW) * gk::WT && p.nres2 == n2;
        // ... with the head of its ring carried across the all-gather (single-rank launches:
        // res_plan clears it on N ranks)
        p.carry = p.pipe && (tune_carry < 0 || tune_carry != 0) ? gk::PIPE_CARRY : 0;
        return;
    } else {
        p.G = gmax;
        p.r2 = RES_R2_BIG;
        const i64 dt = gk::RT, regs = (i64)p.G * RES_R2_BIG * dt;
        p.l2 = n2 / dt * dt > regs ? RES_L2 : 0;
        spread(dt, RES_R2_BIG, p.l2);
    }
    p.lds = std::max<int>(RES_LDS_MIN, p.l2 * (p.cw ? gk::RT - 64 : gk::RT) * (int)sizeof(double2));
    p.wt = gk::RT;
    p.nt = nt;
}

// Non-temporal Krylov-column loads once a vector of the largest slab no longer
// fits comfortably beside them in the 256 MiB Infinity Cache (set_geometry).
bool nt_auto_for(i64 max_nloc) { return max_nloc * 8 > (i64)48 * 1024 * 1024; }

void plan_info(const ResPlan &p, bool on, long long *info) {
    for (int k = 0; k < GK_RES_INFO_LEN; ++k) info[k] = 0;
    if (!on) return;
    info[RPI_VARIANT] = p.bvar >= 0 ? GK_RES_BLOCKED
                        : p.pc    ? GK_RES_WCOL
                                  : (p.wo ? GK_RES_WONLY
                                          : (p.pf ? GK_RES_PREFETCH : (p.l2 > 0 ? GK_RES_PAIRS_LDS : GK_RES_PAIRS)));
    info[RPI_BLK] = p.bvar >= 0 ? p.blk : 1;
    info[RPI_G] = p.G;
    info[RPI_R2] = p.r2;
    info[RPI_L2] = p.l2;
    info[RPI_PF] = p.pf;
    info[RPI_CW] = p.cw;
    info[RPI_WO] = p.wo;
    info[RPI_NT] = p.nt;
    info[RPI_R2E] = p.r2e;
    info[RPI_L2E] = p.l2e;
    info[RPI_LDS] = p.lds;
    info[RPI_NRES2] = p.nres2;
    info[RPI_WT] = p.wt;
    info[RPI_PIPE] = p.pipe;
    info[RPI_CARRY] = p.carry;
}

// -------------------------------------------------------------- launchers ---
int fail(std::string &msg, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return code;
}

int dyn_lds(const void *kernel, int dev, int lds, std::atomic<int> *memo, std::string &msg) {
    if (dev < 0 || dev >= ATTR_DEVS) return fail(msg, GK_ERR_ARG, "device id %d out of range", dev);
    const hipError_t e = ensure_dyn_lds(kernel, dev, lds, memo);
    if (e != hipSuccess)
        return fail(msg, GK_ERR_HIP, "%s:%d hipFuncSetAttribute(dynamic LDS %d): %s", __FILE__, __LINE__, lds,
                    hipGetErrorString(e));
    return GK_OK;
}

int launched(const char *what, std::string &msg) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(msg, GK_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
    return GK_OK;
}

namespace {

template <int R2, int L2, bool PF, bool NT, bool CW, int MODE>
int launch_res_m(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    static std::atomic<int> attr[ATTR_DEVS];
    const int e = dyn_lds(reinterpret_cast<const void *>(&k_mgs_res<R2, L2, PF, NT, CW, MODE>), dev, p.lds, attr, msg);
    if (e != GK_OK) return e;
    k_mgs_res<R2, L2, PF, NT, CW, MODE><<<p.G, RT, p.lds, st>>>(a);
    return launched("resident step", msg);
}

template <int R2, int L2, bool PF, bool NT, bool CW>
int launch_res_t(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    switch (a.mode) {
        case RES_HH_UP: return launch_res_m<R2, L2, PF, NT, CW, RES_HH_UP>(p, a, dev, st, msg);
        case RES_HH_DOWN: return launch_res_m<R2, L2, PF, NT, CW, RES_HH_DOWN>(p, a, dev, st, msg);
        default: return launch_res_m<R2, L2, PF, NT, CW, RES_MGS>(p, a, dev, st, msg);
    }
}

template <int MODE, bool PIPE = false, int CARRY = 0>
int launch_wres_m(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    constexpr int RW = MODE == RES_MGS ? RES_RW : RES_RW_HH;
    constexpr int LW = MODE == RES_MGS ? RES_LW : RES_LW_HH;
    constexpr int WBT = PIPE ? PIPE_D : (MODE == RES_MGS ? WB : WB_HH);
    static std::atomic<int> attr[ATTR_DEVS];
    const int e =
        dyn_lds(reinterpret_cast<const void *>(&k_mgs_wres<RW, LW, MODE, WBT, PIPE, CARRY>), dev, p.lds, attr, msg);
    if (e != GK_OK) return e;
    k_mgs_wres<RW, LW, MODE, WBT, PIPE, CARRY><<<p.G, WT, p.lds, st>>>(a);
    return launched("resident step", msg);
}

int launch_wres(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    switch (a.mode) {
        case RES_HH_UP: return launch_wres_m<RES_HH_UP>(p, a, dev, st, msg);
        case RES_HH_DOWN: return launch_wres_m<RES_HH_DOWN>(p, a, dev, st, msg);
        default:
            if constexpr (RES_PIPE_OK) {
                if (p.pipe) {
                    // the counted waits of the pipelined pass hold on full workgroups only
                    if (p.r2e != RES_RW || p.l2e != RES_LW || (a.n & 1) || a.nres2 != a.n / 2)
                        return fail(msg, GK_ERR_STATE, "pipelined w-only step on a plan that is not full (%d + %d chunks)",
                                    p.r2e, p.l2e);
                    if constexpr (PIPE_CARRY > 0) {
                        // (N ranks: the pushers drain vmcnt before they publish, which would put
                        // the carried loads on every rank's critical path)
                        if (p.carry != 0) {
                            if (a.nranks != 1 || p.carry != PIPE_CARRY)
                                return fail(msg, GK_ERR_STATE, "carried pass (%d chunks) on %d ranks", p.carry, a.nranks);
                            return launch_wres_m<RES_MGS, true, PIPE_CARRY>(p, a, dev, st, msg);
                        }
                    }
                    return launch_wres_m<RES_MGS, true>(p, a, dev, st, msg);
                }
            }
            return launch_wres_m<RES_MGS>(p, a, dev, st, msg);
    }
}

template <int RW, int RX, int LX, int MODE>
int launch_wpc_k(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    constexpr int WBT = MODE == RES_MGS ? RES_PC_WB : RES_PC_WB_HH;
    static std::atomic<int> attr[ATTR_DEVS];
    if (p.r2e > RW || p.lds < LX * RES_PC_NT * (int)sizeof(double2))
        return fail(msg, GK_ERR_STATE, "column-cache plan (%d chunks, %d B LDS) does not fit k_mgs_wpc<%d,%d,%d>", p.r2e,
                    p.lds, RW, RX, LX);
    const int e = dyn_lds(reinterpret_cast<const void *>(&k_mgs_wpc<RW, RX, LX, MODE, WBT, RES_PC_NT>), dev,
                          p.lds, attr, msg);
    if (e != GK_OK) return e;
    k_mgs_wpc<RW, RX, LX, MODE, WBT, RES_PC_NT><<<p.G, RES_PC_NT, p.lds, st>>>(a);
    return launched("resident step", msg);
}

template <int MODE>
int launch_wpc_m(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    if constexpr (RES_PCS) {
        if (p.pcs) return launch_wpc_k<RES_PCS_RW, RES_PCS_RX, RES_PCS_LX, MODE>(p, a, dev, st, msg);
    }
    return launch_wpc_k<RES_PC_RW, MODE == RES_MGS ? RES_PC_RX_MGS : RES_PC_RX, RES_PC_LX, MODE>(p, a, dev, st, msg);
}

}  // namespace

int res_launch(const ResPlan &p, const ResArgs &a, int dev, hipStream_t st, std::string &msg) {
    if (p.bvar >= 0) {
        if (a.mode != RES_MGS) return fail(msg, GK_ERR_STATE, "the blocked step is the MGS-R step's only");
        return blk_launch(p.bvar, p.blk, a, p.G, p.lds, dev, st, msg);
    }
    if (p.wo) return launch_wres(p, a, dev, st, msg);
    if (p.pc) {
        switch (a.mode) {
            case RES_HH_UP: return launch_wpc_m<RES_HH_UP>(p, a, dev, st, msg);
            case RES_HH_DOWN: return launch_wpc_m<RES_HH_DOWN>(p, a, dev, st, msg);
            default: return launch_wpc_m<RES_MGS>(p, a, dev, st, msg);
        }
    }
#define GK_RES_CASE(R, L, PFV, CWV)                                           \
    if (p.r2 == R && p.l2 == L && p.pf == PFV && p.cw == CWV)                \
        return p.nt ? launch_res_t<R, L, PFV, true, CWV>(p, a, dev, st, msg) \
                    : launch_res_t<R, L, PFV, false, CWV>(p, a, dev, st, msg);
    GK_RES_CASE(2, 0, true, true)
    GK_RES_CASE(4, 0, true, true)
    GK_RES_CASE(8, 0, true, true)
    GK_RES_CASE(RES_R2_BIG, 0, false, false)
    GK_RES_CASE(RES_R2_BIG, RES_L2, false, false)
#undef GK_RES_CASE
    return fail(msg, GK_ERR_ARG, "no resident variant for r2=%d l2=%d", p.r2, p.l2);
}

}  // namespace gk
