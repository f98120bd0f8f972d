// gk_api.hip -- C-ABI implementation of include/gmres_hip.h (libgmres_hip.so): the
// context, the Arnoldi steps, tuning and profiling.  The operator and the preconditioner
// live in gk_op.hip, the collectives in gk_comm.hip, the resident step's kernels,
// planner and launchers in gk_resident.hip (the blocked step in gk_blk.hip), the
// short-recurrence solvers in gk_sr_api.hip; gk_host.hpp is what they share.
//
// One context per GPU (one process per GPU on a node).  A context owns the
// slab of grid lines [line0, line0+nlines) of every vector, the Krylov basis
// V (n_loc x (m+1), column stride padded to 256 B) and the reduction slabs,
// all resident in HBM for the whole solve; the host sees only the (j+1)
// Hessenberg entries of each Arnoldi step.  All work is issued on one HIP
// stream per context; on N GPUs the dot-product slabs are RCCL all-reduced
// and the stencil halos exchanged point-to-point on that same stream.
#include <dlfcn.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gk_blk.hpp"
#include "gk_cb.hpp"
#include "gk_cgs.hpp"
#include "gk_host.hpp"
#include "gk_kernels.hpp"
#include "gk_mg.hpp"
#include "gk_resident.hpp"

using namespace gkh;
using gk::nt_auto_for;
using gk::plan_info;
using gk::plan_resident;
using gk::ResPlan;
using gk::RES_R2_BIG;

namespace gkh __attribute__((visibility("hidden"))) {

thread_local std::string g_err;

int set_err(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

i64 round_up(i64 a, i64 b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------- profiling ---
int prof_harvest(gk_ctx *c) {
    if (c->nev == 0) return GK_OK;
    HIPCHK(hipEventSynchronize(c->ev1[c->nev - 1]));
    for (int k = 0; k < c->nev; ++k) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0[k], c->ev1[k]));
        c->prof_ms[c->evk[k]] += ms;
        c->prof_n[c->evk[k]] += 1;
    }
    c->nev = 0;
    return GK_OK;
}

// Captured launch-path steps hold kernel arguments and communicator calls of the
// configuration they were captured in: any change of tuning, preconditioner or
// communicator drops them.
void graph_reset(gk_ctx *c) {
    for (hipGraphExec_t &g : c->gstep)
        if (g != nullptr) {
            (void)hipGraphExecDestroy(g);
            g = nullptr;
        }
    c->gkey = -1;
    if (c->sr_graph != nullptr) {
        (void)hipGraphExecDestroy(c->sr_graph);
        c->sr_graph = nullptr;
    }
}

// -------------------------------------------------------------- geometry ---
void set_geometry(gk_ctx *c) {
    const int N = c->N;
    c->vec = (N % 2 == 0) ? 2 : 1;
    const int gx = (N + gk::TPB * c->vec - 1) / (gk::TPB * c->vec);
    const int ml = c->max_lines > 0 ? c->max_lines : c->nlines;
    // ~2048 workgroups for the stencil sweeps, marching JT lines each
    const int target = c->tune_st_blocks > 0 ? c->tune_st_blocks : 2048;
    int JT = (int)std::max<i64>(1, ((i64)ml * gx + target - 1) / target);
    if (JT > 64) JT = 64;
    int gy = (ml + JT - 1) / JT;
    while ((i64)gx * gy > gk::NPMAX) {
        ++JT;
        gy = (ml + JT - 1) / JT;
    }
    c->JT = JT;
    c->sgrid = dim3(gx, gy, 1);
    c->np_st = gx * gy;
    {  // the short-recurrence marches: fewer, longer marches (each re-reads 2 neighbour lines per march)
        const int srt = c->tune_sr_blocks > 0 ? c->tune_sr_blocks : 512;
        int sjt = (int)std::max<i64>(1, ((i64)ml * gx + srt - 1) / srt);
        if (sjt > 256) sjt = 256;
        int sgy = (ml + sjt - 1) / sjt;
        while ((i64)gx * sgy > gk::NPMAX) {
            ++sjt;
            sgy = (ml + sjt - 1) / sjt;
        }
        c->sr_JT = sjt;
        c->sr_sgrid = dim3(gx, sgy, 1);
        c->np_sr = gx * sgy;
    }
    // projection kernels: fixed workgroup count derived from the largest slab
    const i64 nmax2 = ((i64)ml * N + 1) / 2;
    i64 npj = (nmax2 + (i64)gk::TPB * gk::UNR - 1) / ((i64)gk::TPB * gk::UNR);
    if (npj > 1024) npj = 1024;
    if (c->tune_pj_blocks > 0) npj = std::min<i64>(c->tune_pj_blocks, gk::NPMAX);
    // Krylov columns by non-temporal loads once a vector no longer fits
    // comfortably beside them in the 256 MiB Infinity Cache (measured: -20 %
    // projection time at 4096^2, +6 % at 1024^2 where everything is resident).
    c->nt_auto = nt_auto_for((i64)ml * N);
    if (npj < 1) npj = 1;
    c->np_pj = (int)npj;
    // elementwise kernels: also from the largest slab (their partial slabs are all-reduced)
    i64 nb = (nmax2 + gk::TPB - 1) / gk::TPB;
    c->nblk_stream = (int)std::min<i64>(std::max<i64>(nb, 1), 2048);
}

// -------------------------------------------------------------- launches ---
// T: the type va / vb are stored in (float: the FP32 basis, PJ_AXPY_DOT / PJ_AXPY_NORM only)
template <bool NT, int U, class T>
void launch_proj_u(gk_ctx *c, int mode, double *w, const T *va, const T *vb, const double *pin, int npin,
                   double *pout, double *hslot, double coef, i64 tail0, int hstore) {
    const dim3 g(c->np_pj);
    const i64 n = c->nloc;
    if constexpr (std::is_same<T, double>::value) {
        if (mode == gk::PJ_DOT) {
            gk::k_proj<gk::PJ_DOT, NT, U><<<g, gk::TPB, 0, c->st>>>(w, va, vb, pin, npin, pout, hslot, coef, n,
                                                                    tail0, 0, hstore);
            return;
        }
        if (mode == gk::PJ_AXPY) {
            gk::k_proj<gk::PJ_AXPY, NT, U><<<g, gk::TPB, 0, c->st>>>(w, va, vb, pin, npin, pout, hslot, coef, n,
                                                                     tail0, 0, hstore);
            return;
        }
    }
    if (mode == gk::PJ_AXPY_DOT)
        gk::k_proj<gk::PJ_AXPY_DOT, NT, U, T><<<g, gk::TPB, 0, c->st>>>(w, va, vb, pin, npin, pout, hslot, coef, n,
                                                                        tail0, 0, hstore);
    else
        gk::k_proj<gk::PJ_AXPY_NORM, NT, U, T><<<g, gk::TPB, 0, c->st>>>(w, va, vb, pin, npin, pout, hslot, coef, n,
                                                                         tail0, 0, hstore);
}

template <bool NT, class T>
void launch_proj(gk_ctx *c, int mode, double *w, const T *va, const T *vb, const double *pin, int npin,
                 double *pout, double *hslot, double coef, i64 tail0, int hstore) {
    // loads in flight per thread and array: one trip per thread when the vector is small, else 2
    const i64 per_thread = (c->nloc / 2 + (i64)c->np_pj * gk::TPB - 1) / ((i64)c->np_pj * gk::TPB);
    if (per_thread > 4)
        launch_proj_u<NT, 2>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    else
        launch_proj_u<NT, 4>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
}

// (T is named, never deduced: callers pass nullptr for the column a mode does not read)
template <class T = double>
int proj(gk_ctx *c, int mode, double *w, const std::common_type_t<T> *va, const std::common_type_t<T> *vb,
         const double *pin, int npin, double *pout, double *hslot, double coef, i64 tail0 = 0, int hstore = 0) {
    if (!std::is_same<T, double>::value && mode != gk::PJ_AXPY_DOT && mode != gk::PJ_AXPY_NORM)
        return set_err(GK_ERR_STATE, "projection mode %d on float columns", mode);
    ProfScope ps(c, GK_KID_PROJ);
    if (c->tune_nt > 0 || (c->tune_nt < 0 && c->nt_auto))
        launch_proj<true>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    else
        launch_proj<false>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    LAUNCHCHK();
    return GK_OK;
}

int scale(gk_ctx *c, double *out, const double *w, const double *pin, int npin, double *hslot,
          double *hcopy = nullptr, const double *hsrc = nullptr, int ncopy = 0, bool pin_norm = false) {
    ProfScope ps(c, GK_KID_SCALE);
    gk::k_scale<<<c->nblk_stream, gk::TPB, 0, c->st>>>(out, w, pin, npin, hslot, c->nloc, hcopy, hsrc, ncopy,
                                                       pin_norm ? 1 : 0);
    LAUNCHCHK();
    return GK_OK;
}

// V(:,k+1) = w / h, h = sqrt(sum(pin)), in the basis' own type; the FP32 basis also widens the
// new column to vjw (the operator's next input) and, for column 1, to v1w (the first dot's partner)
int scale_col(gk_ctx *c, int k, const double *pin, int npin, double *hslot, double *hcopy = nullptr,
              const double *hsrc = nullptr, int ncopy = 0) {
    if (!cb_on(c)) return scale(c, vcol<double>(c, k), c->w, pin, npin, hslot, hcopy, hsrc, ncopy);
    ProfScope ps(c, GK_KID_SCALE);
    HIPCHK(gk::cb_scale(c->nblk_stream, vcol<float>(c, k), cb_vjw(c), k == 0 ? cb_v1w(c) : nullptr, c->w, pin, npin,
                        hslot, c->nloc, hcopy, hsrc, ncopy, c->st));
    return GK_OK;
}

// x (+)= V(:, 1:n_out) ydev on the basis as it is stored
template <bool ADD, class T>
void launch_update_x(gk_ctx *c, double *x, int n_out) {
    gk::k_update_x<ADD, T><<<c->nblk_stream, gk::TPB, 0, c->st>>>(x, vcol<T>(c, 0), c->ld, c->ydev, n_out, c->nloc);
}
template <bool ADD>
int update_x(gk_ctx *c, double *x, int n_out) {
    ProfScope ps(c, GK_KID_UPDATE);
    cb_on(c) ? launch_update_x<ADD, float>(c, x, n_out) : launch_update_x<ADD, double>(c, x, n_out);
    LAUNCHCHK();
    return GK_OK;
}

// x += w: the last launch of the updates that do not end in update_x<true>
int add_into(gk_ctx *c, double *x, const double *w) {
    ProfScope ps(c, GK_KID_UPDATE);
    gk::k_add<<<c->nblk_stream, gk::TPB, 0, c->st>>>(x, w, c->nloc);
    LAUNCHCHK();
    return GK_OK;
}

// NORM2 of x(0:n) in flang-rt's order into out[0] (GK_TUNE_HH_NORM_ORDER)
int norm2_seq(gk_ctx *c, const double *x, i64 n, double *out) {
    ProfScope ps(c, GK_KID_OTHER);
    gk::k_norm2_seq<<<1, gk::TPB, 0, c->st>>>(x, n, out);
    LAUNCHCHK();
    return GK_OK;
}

int fill_hash(gk_ctx *c, double *x, unsigned long long seed) {
    gk::k_fill_hash<<<c->nblk_stream, gk::TPB, 0, c->st>>>(x, c->nloc, c->g0, seed);
    LAUNCHCHK();
    return GK_OK;
}

int finalize(gk_ctx *c, const double *pin, int npin, double *out, int take_sqrt) {
    ProfScope ps(c, GK_KID_OTHER);
    gk::k_finalize<<<1, gk::TPB, 0, c->st>>>(pin, npin, out, take_sqrt);
    LAUNCHCHK();
    return GK_OK;
}

// Can step j run as one resident launch, and with which variant?  Needs an
// in-launch reduction path: single rank, or the device exchange (RCCL and the
// host-side local group cannot be driven from inside a kernel).
bool res_plan(gk_ctx *c, ResPlan &p, bool hh = false) {
    if (c->tune_res == 0 || c->res_broken || c->m > gk::RHMAX || c->res_cus <= 0 || c->res_gath == nullptr)
        return false;
    if (collective(c) && !(c->xs_on && c->nranks > 1)) return false;
    // Several resident launches on one device spin on each other's partials, so
    // their streams must run concurrently -- HIP promises nothing about how
    // streams map to hardware queues.  Auto mode assumes one context per device.
    if (c->tune_res < 0 && c->res_share > 1) return false;
    const int gmax = std::max(1, std::min(gk::RGMAX, c->res_cus / std::max(1, c->res_share)));
    const int cap = c->tune_res_r2 > 0 ? c->tune_res_r2 : RES_R2_BIG;
    plan_resident(c->nloc, gmax, cap, c->tune_res_wonly, hh,
                  c->tune_nt > 0 || (c->tune_nt < 0 && c->nt_auto), p, c->tune_res_pc, c->tune_res_blk, c->tune_res_pf,
                  c->tune_res_pipe, c->tune_res_carry);
    if (c->nranks > 1) p.carry = 0;  // the carried pass is the single-rank launches' (gk_resident.hip)
    if (p.wo && !hh && c->m + 1 > gk::WO_HMAX) return false;  // its H column: WO_HMAX entries of LDS
    return true;
}

// One resident launch (gk::ResArgs::mode):
//  RES_MGS: the MGS cascade of step j + norm + scale; pin/npin = the
//    (all-reduced) partial slab of the first dot <w, V(:,1)>; H column to hs/hcopy.
//  RES_HH_UP: w = P_j..P_1 w (pin = <w, P_1>); hs[0] = ||w(j+1:n)||^2.
//  RES_HH_DOWN: w = P_1..P_j w (no pin).
//  flags (w-only variant, p.wo): RESF_CLOSE_HH -- RES_HH_UP also makes P(:,j+1) and
//    writes w(1:j+1) to c->hb (one more exchange); RESF_UNIT_INIT -- RES_HH_DOWN builds
//    its unit input e_{unit_g} itself.
enum { RESF_CLOSE_HH = 1, RESF_UNIT_INIT = 2, RESF_PIN_LOCAL = 4 };

// What a resident launch of step j with np exchanges takes from the context, whichever
// basis it runs on (Plan: ResPlan or gk::CbPlan): w, the first dot's slab, the H column's
// two destinations, the plan's split of w, the all-gather's granule region, tags and
// timeout, the error word, the stamps and the trace hook -- for one rank.
template <class Plan>
int res_args(gk_ctx *c, int j, int mode, const Plan &p, int np, const double *pin, int npin, double *hs,
             double *hcopy, gk::ResArgs &a) {
    if (c->res_tag > 0xF0000000u) {  // tags must never repeat within the granule region's lifetime
        HIPCHK(hipMemsetAsync(c->res_gath, 0, sizeof(gk::u64) * gk::RES_GATH_ALL, c->st));
        c->res_tag = 1;
    }
    a.w = c->w;
    a.mode = mode;
    a.coef = mode == gk::RES_MGS ? 1.0 : 2.0;
    a.ld = c->ld;
    a.pin = pin;
    a.npin = npin;
    a.hs = hs;
    a.hcopy = hcopy;
    a.gath = c->res_gath;
    a.j = j;
    a.n = c->nloc;
    a.nres2 = p.nres2;
    a.r2e = p.r2e;
    a.l2e = p.l2e;
    a.tag0 = c->res_tag;
    c->res_tag += (unsigned)np;
    a.timeout = (gk::u64)c->res_timeout_ms * (gk::u64)c->xs_tick_per_ms;
    a.err = c->res_err_dev;
    a.stamps = c->res_split ? c->res_stamps : nullptr;
    if (c->res_trace != nullptr && j == c->res_trace_j && mode == c->res_trace_mode) {
        a.trace = c->res_trace;
        c->res_trace_g = p.G;
        c->res_trace_np = np;
    }
    a.nranks = 1;
    return GK_OK;
}

int res_step(gk_ctx *c, int j, const ResPlan &p, const double *pin, int npin, double *hs, double *hcopy,
             int mode = gk::RES_MGS, double *w = nullptr, i64 unit_g = -1, int flags = 0) {
    ProfScope ps(c, GK_KID_RES);
    const bool close = (flags & RESF_CLOSE_HH) && mode == gk::RES_HH_UP;
    if ((flags & ~RESF_PIN_LOCAL) != 0 && !p.wo)
        return set_err(GK_ERR_STATE, "resident flags %d need the w-only variant", flags);
    const bool pin_local = (flags & RESF_PIN_LOCAL) && mode != gk::RES_HH_DOWN && c->xs_on && c->nranks > 1;
    // exchanges of the launch
    const int np = (mode == gk::RES_MGS ? (p.bvar >= 0 ? gk::blk_exchanges(j, p.blk) : 2 * j) : j) + (close ? 1 : 0);
    gk::ResArgs a{};
    CHK(res_args(c, j, mode, p, np, pin, npin, hs, hcopy, a));
    if (w != nullptr) a.w = w;
    a.tail0 = mode == gk::RES_HH_UP ? (i64)j - c->g0 : 0;
    a.V = c->V;
    a.vout = c->V + (i64)j * c->ld;
    a.gm = c->res_gm;
    a.unit_known = mode == gk::RES_HH_DOWN && unit_g >= 0;
    a.unit_e = (a.unit_known && unit_g >= c->g0 && unit_g < c->g0 + c->nloc) ? unit_g - c->g0 : -1;
    a.unit_init = a.unit_known && (flags & RESF_UNIT_INIT) ? 1 : 0;
    a.close_hh = close ? 1 : 0;
    a.hb = c->hb;
    // auto: on -- A/B at 2896^2 (k_mgs_res<12, 18> NT, profiles/r04/ab_qdef_2896_r04a.jsonl): 19.98 /
    // 19.90 -> 18.82 / 18.84 us per projection
    a.qdef = c->tune_res_qdef != 0 ? 1 : 0;
    if (c->xs_on && c->nranks > 1) {
        a.err = c->xs_err_dev;
        a.timeout = std::max(a.timeout, c->xs_timeout);
        a.peers = c->xs_peers;
        a.nranks = c->nranks;
        a.rank = c->rank;
        a.pin_local = pin_local ? 1 : 0;  // the first dot's rank hop takes the launch's first number
        a.xseq0 = c->xs_seq + (pin_local ? 1u : 0u);
        c->xs_seq += (unsigned)np + (pin_local ? 1u : 0u);
    }
    std::string msg;
    const int e = gk::res_launch(p, a, c->dev, c->st, msg);
    return e == GK_OK ? GK_OK : set_err(e, "%s", msg.c_str());
}

// Compressed basis (gk_set_basis_precision GK_BASIS_F32): can step j run as one resident
// launch of k_mgs_wcb?  Single rank by construction; the blocked / prefetching steps do
// not exist on float columns (GK_TUNE_RES_BLOCK, GK_TUNE_RES_PF ignored).
bool cb_plan_ctx(gk_ctx *c, gk::CbPlan &p) {
    if (c->tune_res == 0 || c->res_broken || c->res_cus <= 0 || c->res_gath == nullptr || c->nranks > 1) return false;
    if (c->tune_res < 0 && c->res_share > 1) return false;  // (as res_plan: auto assumes one context per device)
    gk::plan_cb(c->nloc, c->res_cus, c->res_share, c->m, p);
    return p.on;
}

// The resident launch of step j on float columns (2 j exchanges): res_step's RES_MGS arguments.
int cb_step(gk_ctx *c, int j, const gk::CbPlan &p, const double *pin, int npin, double *hs, double *hcopy) {
    ProfScope ps(c, GK_KID_RES);
    gk::ResArgs a{};
    CHK(res_args(c, j, gk::RES_MGS, p, 2 * j, pin, npin, hs, hcopy, a));
    std::string msg;
    const int e = gk::cb_launch(p, a, vcol<float>(c, 0), cb_vjw(c), c->dev, c->st, msg);
    return e == GK_OK ? GK_OK : set_err(e, "%s", msg.c_str());
}

int d2h_sync(gk_ctx *c, double *host, const double *dev, int count) {
    HIPCHK(hipMemcpyAsync(c->hcol_host, dev, sizeof(double) * count, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    std::memcpy(host, c->hcol_host, sizeof(double) * count);
    return GK_OK;
}

int owner_of(gk_ctx *c, i64 gidx) {
    // ranks own consecutive slabs; rank r owns [g0_r, g0_r + nloc_r). Only the
    // HH path needs this and only for gidx <= m, which lives on the rank whose
    // slab starts at line 0 when N >= m+1 (checked at cycle start).
    (void)gidx;
    return 0;
}

int check_ctx(gk_ctx *c) {
    if (c == nullptr) return set_err(GK_ERR_ARG, "null context");
    if (c->broken)
        return set_err(GK_ERR_STATE, "context broken by an earlier watchdog timeout (work never completed on its "
                                     "stream): destroy it");
    if (c->nranks > 1 && !c->comm_ok) return set_err(GK_ERR_STATE, "communicator not initialised");
    return GK_OK;
}

// The orthogonality diagnostics in the reference's summation order (one running
// sum per dot, gk::seq_dot) unless tuned off; a running sum cannot cross a slab
// boundary without serialising the ranks, so N ranks use the tree (k_gram).
bool verr_ref_order(const gk_ctx *c) { return c->tune_verr_order != 0 && c->nranks == 1; }

int ensure_gram(gk_ctx *c, int ncols) {
    if (ncols > gk::GCMAX) return set_err(GK_ERR_ARG, "v_err needs <= %d columns", gk::GCMAX);
    if (c->gram_slab == nullptr) {
        c->gram_nblk = 512;
        const int maxpairs = gk::GCMAX * (gk::GCMAX + 1) / 2;
        HIPCHK(hipMalloc(&c->gram_slab, sizeof(double) * (size_t)c->gram_nblk * maxpairs));
        HIPCHK(hipMalloc(&c->gram_out, sizeof(double) * maxpairs));
        HIPCHK(hipMalloc(&c->gram_pairs, sizeof(short2) * maxpairs));
    }
    return GK_OK;
}

// k_gram of the first ncols columns of base, stored as T, into the context's slab
template <class T>
void gram_slab(gk_ctx *c, const T *base, int ncols, int np) {
    gk::k_gram<T><<<c->gram_nblk, gk::TPB, 0, c->st>>>(base, c->ld, ncols, c->nloc, c->gram_pairs, np, c->gram_slab);
}

// G (host, c x c symmetric, column-major) of the first c columns of base.
int gram(gk_ctx *c, const double *base, int ncols, std::vector<double> &G) {
    CHK(ensure_gram(c, ncols));
    std::vector<short2> pr;
    for (int bb = 0; bb < ncols; ++bb)
        for (int aa = 0; aa <= bb; ++aa) pr.push_back(make_short2((short)aa, (short)bb));
    const int np = (int)pr.size();
    HIPCHK(hipMemcpyAsync(c->gram_pairs, pr.data(), sizeof(short2) * np, hipMemcpyHostToDevice, c->st));
    const bool f32 = cb_on(c) && base == c->V;  // float columns: the tree (no reference to match in its order)
    if (!f32 && verr_ref_order(c)) {  // one running sum per pair, k in order (the reference's dot_product)
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_seqdot_pairs<<<(np + 63) / 64, 64, 0, c->st>>>(base, c->ld, c->nloc, c->gram_pairs, np, c->gram_out);
        LAUNCHCHK();
    } else {
        ProfScope ps(c, GK_KID_OTHER);
        f32 ? gram_slab(c, vcol<float>(c, 0), ncols, np) : gram_slab(c, base, ncols, np);
        LAUNCHCHK();
        gk::k_gram_reduce<<<(np + gk::TPB - 1) / gk::TPB, gk::TPB, 0, c->st>>>(c->gram_slab, c->gram_nblk,
                                                                            np, c->gram_out);
        LAUNCHCHK();
        CHK(allreduce(c, c->gram_out, np, true));
    }
    std::vector<double> flat(np);
    HIPCHK(hipMemcpyAsync(flat.data(), c->gram_out, sizeof(double) * np, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    G.assign((size_t)ncols * ncols, 0.0);
    for (int p = 0; p < np; ++p) {
        G[(size_t)pr[p].y * ncols + pr[p].x] = flat[p];
        G[(size_t)pr[p].x * ncols + pr[p].y] = flat[p];
    }
    return GK_OK;
}

// v <- P_1 .. P_k v  (apply reflections k..1; hh_step :269-283, update :361-373,
// calculate_verr :581-585).  The chain's first launch is a pure dot.
// unit_g >= 0: v is the unit vector e at global index unit_g (gk_hh_step's v_j,
// calculate_verr's columns), so the chain's leading dot <e, P_k> is the single
// element P_k(unit_g) -- exactly what the full dot sums to -- and the resident
// launch skips that pass.
int reflect_chain_down(gk_ctx *c, double *v, int k, i64 unit_g = -1, int flags = 0) {
    double *P = c->V;
    ResPlan rp;
    if (res_plan(c, rp, true))
        return res_step(c, k, rp, nullptr, 0, nullptr, nullptr, gk::RES_HH_DOWN, v, unit_g, flags);
    if (flags != 0) return set_err(GK_ERR_STATE, "resident chain flags without a resident plan");
    int s0 = 0, s1 = 1;
    CHK(proj(c, gk::PJ_DOT, v, nullptr, P + (i64)(k - 1) * c->ld, nullptr, 0, slot(c, s0), nullptr, 2.0));
    int np = c->np_pj;
    for (int i = k; i >= 1; --i) {
        CHK(allreduce(c, slot(c, s0), np));
        const double *va = P + (i64)(i - 1) * c->ld;
        if (i > 1) {
            CHK(proj(c, gk::PJ_AXPY_DOT, v, va, P + (i64)(i - 2) * c->ld, slot(c, s0), np, slot(c, s1),
                     nullptr, 2.0));
            std::swap(s0, s1);
        } else {
            CHK(proj(c, gk::PJ_AXPY, v, va, nullptr, slot(c, s0), np, nullptr, nullptr, 2.0));
        }
    }
    return GK_OK;
}

// The launch path's MGS-R cascade of step j after the operator launch left the
// first dot's partial slab (np partials) in slot 0: two passes of j projections
// (AXPY_i fused with dot_{i+1}), each dot all-reduced, then h = ||w|| and
// V(:,j+1) = w / h with H(1:j+1, j) published to mapped host memory.
// gmres_mgsr.f90:341-363, :384.
// T: the type the basis is stored in; the FP32 basis' closing also writes vjw (scale_col).
template <class T>
int mgs_chain_t(gk_ctx *c, int j, int np) {
    const int m2 = c->m + 2;
    double *hs = c->hall + (i64)(j - 1) * m2;
    int s0 = 0, s1 = 1;
    const int np_total = 2 * j;
    for (int p = 0; p < np_total; ++p) {
        const int i = p % j;
        CHK(allreduce(c, slot(c, s0), np));
        const T *va = vcol<T>(c, i);
        const int first_pass = p < j;
        if (p + 1 < np_total) {
            const T *vb = vcol<T>(c, (p + 1) % j);
            CHK(proj<T>(c, gk::PJ_AXPY_DOT, c->w, va, vb, slot(c, s0), np, slot(c, s1), hs + i, 1.0, 0, first_pass));
        } else {
            CHK(proj<T>(c, gk::PJ_AXPY_NORM, c->w, va, nullptr, slot(c, s0), np, slot(c, s1), hs + i, 1.0, 0,
                        first_pass));
        }
        np = c->np_pj;
        std::swap(s0, s1);
    }
    CHK(allreduce(c, slot(c, s0), np));
    return scale_col(c, j, slot(c, s0), np, hs + j, c->hallh_dev + (i64)(j - 1) * m2, hs, j);
}

// The CGS2 step's buffers, allocated at its first use: the dots' partial slab (m rows of
// np_pj workgroups) and s (m doubles).  A slab grown for a larger workgroup count drops the
// captured steps, which hold its address.
int ensure_cgs(gk_ctx *c) {
    const i64 need = (i64)c->m * c->np_pj;
    if (c->cgs_slab == nullptr || c->cgs_cap < need) {
        graph_reset(c);
        if (c->cgs_slab != nullptr) HIPCHK(hipFree(c->cgs_slab));
        c->cgs_slab = nullptr;
        c->cgs_cap = 0;
        HIPCHK(hipMalloc(&c->cgs_slab, sizeof(double) * (size_t)need));
        c->cgs_cap = need;
    }
    if (c->cgs_s == nullptr) HIPCHK(hipMalloc(&c->cgs_s, sizeof(double) * (size_t)c->m));
    return GK_OK;
}

// The CGS2 cascade of step j (gk_set_orthogonalization GK_ORTH_CGS2, gk_cgs.hpp) after the
// operator launch: two sweeps of batched dots on the same w, their fixed-order reduce, the
// all-reduce of s and the j-column AXPY (the second also leaves the partials of ||w||^2),
// then the MGS-R step's closing.  7 launches and 3 all-reduces whatever j is.
int cgs_chain(gk_ctx *c, int j) {
    const int m2 = c->m + 2, G = c->np_pj;
    double *hs = c->hall + (i64)(j - 1) * m2;
    const bool nt = c->tune_nt > 0 || (c->tune_nt < 0 && c->nt_auto);
    if (c->cgs_slab == nullptr || c->cgs_s == nullptr || c->cgs_cap < (i64)j * G)
        return set_err(GK_ERR_STATE, "CGS2 step %d without its buffers", j);
    for (int sweep = 0; sweep < 2; ++sweep) {
        {
            ProfScope ps(c, GK_KID_PROJ);
            HIPCHK(gk::cgs_dots(c->cgs_kb, nt, G, c->w, c->V, c->ld, j, c->nloc, c->cgs_slab, c->st));
        }
        {
            ProfScope ps(c, GK_KID_OTHER);
            HIPCHK(gk::cgs_reduce(c->cgs_slab, G, j, c->cgs_s, c->st));
        }
        CHK(allreduce(c, c->cgs_s, j, true));
        {
            ProfScope ps(c, GK_KID_PROJ);
            HIPCHK(gk::cgs_axpy(sweep == 1, nt, G, c->w, c->V, c->ld, j, c->nloc, c->cgs_s, hs, sweep == 0, slot(c, 0),
                                c->st));
        }
    }
    CHK(allreduce(c, slot(c, 0), G));
    return scale_col(c, j, slot(c, 0), G, hs + j, c->hallh_dev + (i64)(j - 1) * m2, hs, j);
}

// The launch-path chain of step j the context's scheme selects (np: the first dot's partials,
// which the CGS2 chain does not consume).
int mgs_chain(gk_ctx *c, int j, int np) {
    if (cgs_on(c)) return cgs_chain(c, j);
    return cb_on(c) ? mgs_chain_t<float>(c, j, np) : mgs_chain_t<double>(c, j, np);
}

// Capture mgs_chain(j) once as a graph (its kernel arguments and communicator
// calls depend only on j, np and the context's fixed buffers).  A capture that
// fails switches graphs off for this context; one rank then runs the step call by
// call.  With an RCCL communicator the failure is an error instead: the discarded
// graph may already hold some of the step's ncclAllReduce calls, and whether RCCL's
// per-communicator operation counters stay matched when one rank runs eagerly while
// its peers replay is not pinned -- the caller reruns with GK_TUNE_GRAPH 0 on every
// rank.  (GK_DEBUG_CAPTURE_FAIL=1 makes every capture fail after it ends, for tests.)
int capture_step(gk_ctx *c, int j, int np) {
    HIPCHK(hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    c->graph_seq0 = c->xs_seq;
    const int rc = mgs_chain(c, j, np);
    c->capturing = false;
    const unsigned nxs = c->xs_seq - c->graph_seq0;  // nothing ran: the numbers are reused by the replay
    c->xs_seq = c->graph_seq0;
    if ((int)c->gxs.size() < c->m + 1) c->gxs.resize(c->m + 1, 0);
    c->gxs[j] = nxs;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->st, &g);
    hipGraphExec_t ge = nullptr;
    hipError_t e2 = hipErrorUnknown;
    if (rc == GK_OK && e == hipSuccess && g != nullptr) e2 = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (g != nullptr) (void)hipGraphDestroy(g);
    const char *dbg = std::getenv("GK_DEBUG_CAPTURE_FAIL");
    const bool forced = dbg != nullptr && dbg[0] == '1';
    if (rc != GK_OK || e != hipSuccess || e2 != hipSuccess || forced) {
        const std::string why = rc != GK_OK ? g_err
                                : forced   ? std::string("GK_DEBUG_CAPTURE_FAIL")
                                           : hipGetErrorString(e != hipSuccess ? e : e2);
        (void)hipGetLastError();
        if (ge != nullptr) (void)hipGraphExecDestroy(ge);
        c->tune_graph = 0;
        graph_reset(c);
        if (c->comm != nullptr && !c->xs_on && c->lg == nullptr)  // the step's all-reduces are RCCL calls
            return set_err(GK_ERR_COMM,
                           "capture of launch-path step %d failed on an RCCL rank (%s): rerun with GK_TUNE_GRAPH 0 "
                           "on every rank (one rank running the step eagerly while its peers replay graphs is not "
                           "supported)", j, why.c_str());
        set_err(GK_OK, "launch-path step graphs off for this context: capture of step %d failed (%s)", j,
                why.c_str());
        return GK_OK;
    }
    c->gstep[j] = ge;
    return GK_OK;
}

}  // namespace gkh

// ======================================================================= API

extern "C" {

const char *gk_last_error(void) { return g_err.c_str(); }
int gk_version(void) { return 1; }

int gk_runtime_info(int *hip_runtime, int *hip_driver, int *rccl, char *hip_path, char *rccl_path, int len) {
    if (hip_runtime == nullptr || hip_driver == nullptr || rccl == nullptr) return set_err(GK_ERR_ARG, "null argument");
    *hip_runtime = *hip_driver = *rccl = 0;
    HIPCHK(hipRuntimeGetVersion(hip_runtime));
    HIPCHK(hipDriverGetVersion(hip_driver));
    NCCLCHK(ncclGetVersion(rccl));
    auto path_of = [&](const void *sym, char *out) {
        if (out == nullptr || len <= 0) return;
        Dl_info di{};
        const char *p = (dladdr(sym, &di) != 0 && di.dli_fname != nullptr) ? di.dli_fname : "";
        std::snprintf(out, (size_t)len, "%s", p);
    };
    path_of(reinterpret_cast<const void *>(&hipRuntimeGetVersion), hip_path);
    path_of(reinterpret_cast<const void *>(&ncclGetVersion), rccl_path);
    return GK_OK;
}

int gk_create(int device, int nside, int line0, int nlines, int m, gk_ctx **out) {
    if (out == nullptr) return set_err(GK_ERR_ARG, "null out");
    *out = nullptr;
    if (nside < 2 || nlines < 1 || line0 < 0 || line0 + nlines > nside || m < 1 || m > 4096)
        return set_err(GK_ERR_ARG, "bad shape N=%d line0=%d nlines=%d m=%d", nside, line0, nlines, m);
    // GK_CGS_KB (environment, read here): columns a dots workgroup of the CGS2 step batches, for A/B runs
    int cgs_kb = gk::CGS_KB_DEFAULT;
    if (const char *kb = std::getenv("GK_CGS_KB")) {
        cgs_kb = std::atoi(kb);
        if (cgs_kb != 8 && cgs_kb != 16) return set_err(GK_ERR_ARG, "GK_CGS_KB=%s: batches of 8 or 16 columns", kb);
    }
    HIPCHK(hipSetDevice(device));
    gk_ctx *c = new gk_ctx();
    c->cgs_kb = cgs_kb;
    c->dev = device;
    c->N = nside;
    c->line0 = line0;
    c->nlines = nlines;
    c->m = m;
    c->nloc = (i64)nside * nlines;
    c->g0 = (i64)nside * line0;
    c->ld = round_up(c->nloc, 32);  // 256-byte aligned columns
    c->max_lines = nlines;
    set_geometry(c);
    auto fail = [&](int code) {
        gk_destroy(c);
        return code;
    };
    if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess)
        return fail(set_err(GK_ERR_HIP, "stream create failed"));
    const size_t vb = sizeof(double) * (size_t)c->ld;
    if (hipMalloc(&c->V, vb * (m + 1)) != hipSuccess)
        return fail(set_err(GK_ERR_NOMEM, "cannot allocate V: %.2f GB", vb * (m + 1) / 1e9));
    double **vecs[] = {&c->w, &c->z, &c->aux, &c->dA, &c->dB, &c->x, &c->b, &c->vj};
    for (double **p : vecs)
        if (hipMalloc(p, vb) != hipSuccess) return fail(set_err(GK_ERR_NOMEM, "cannot allocate work vectors"));
    if (hipMalloc(&c->hlo, sizeof(double) * nside) != hipSuccess ||
        hipMalloc(&c->hhi, sizeof(double) * nside) != hipSuccess ||
        hipMalloc(&c->dh, sizeof(double) * 6 * gk::CF_HMAX * (size_t)nside) != hipSuccess ||
        hipMalloc(&c->zline, sizeof(double) * (size_t)nside) != hipSuccess ||
        hipMemsetAsync(c->zline, 0, sizeof(double) * (size_t)nside, c->st) != hipSuccess ||
        hipMalloc(&c->red, sizeof(double) * NSLOT * gk::NPMAX) != hipSuccess ||
        hipMalloc(&c->hcol, sizeof(double) * (m + 2)) != hipSuccess ||
        hipMalloc(&c->ydev, sizeof(double) * (m + 1)) != hipSuccess ||
        hipMalloc(&c->hb, sizeof(double) * (m + 2)) != hipSuccess ||
        hipMalloc(&c->scal, sizeof(double) * 8) != hipSuccess)
        return fail(set_err(GK_ERR_NOMEM, "cannot allocate small buffers"));
    if (hipHostMalloc(&c->hcol_host, sizeof(double) * (m + 2 + gk::GCMAX)) != hipSuccess)
        return fail(set_err(GK_ERR_NOMEM, "cannot allocate pinned buffer"));
    if (hipMalloc(&c->hall, sizeof(double) * (size_t)(m + 2) * (m + 1)) != hipSuccess ||
        hipHostMalloc(&c->hallh, sizeof(double) * (size_t)(m + 2) * (m + 1), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->hallh_dev, c->hallh, 0) != hipSuccess)
        return fail(set_err(GK_ERR_NOMEM, "cannot allocate the Hessenberg mirrors"));
    if (hipMalloc(&c->res_gath, sizeof(gk::u64) * gk::RES_GATH_ALL) != hipSuccess ||
        hipMalloc(&c->res_gm, sizeof(double) * (size_t)(m + 1 + gk::RES_SMAX) * gk::RES_SMAX) != hipSuccess ||
        hipHostMalloc((void **)&c->res_err, sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->res_err_dev, c->res_err, 0) != hipSuccess ||
        hipMemsetAsync(c->res_gm, 0, sizeof(double) * (size_t)(m + 1 + gk::RES_SMAX) * gk::RES_SMAX, c->st) != hipSuccess ||
        hipMemsetAsync(c->res_gath, 0, sizeof(gk::u64) * gk::RES_GATH_ALL, c->st) != hipSuccess)
        return fail(set_err(GK_ERR_NOMEM, "cannot allocate the resident-step exchange area"));
    *c->res_err = 0;
    {
        int cus = 0, khz = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) c->res_cus = cus;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
            c->xs_tick_per_ms = khz;
    }
    c->ev_step.assign(m + 1, nullptr);
    for (int k = 0; k <= m; ++k)
        if (hipEventCreateWithFlags(&c->ev_step[k], hipEventDisableTiming) != hipSuccess)
            return fail(set_err(GK_ERR_HIP, "event create failed"));
    if (hipMemsetAsync(c->x, 0, vb, c->st) != hipSuccess || hipMemsetAsync(c->b, 0, vb, c->st) != hipSuccess ||
        hipMemsetAsync(c->V, 0, vb * (m + 1), c->st) != hipSuccess ||
        hipMemsetAsync(c->red, 0, sizeof(double) * NSLOT * gk::NPMAX, c->st) != hipSuccess)
        return fail(set_err(GK_ERR_HIP, "memset failed"));
    c->ev0.resize(PROF_POOL);
    c->ev1.resize(PROF_POOL);
    c->evk.resize(PROF_POOL);
    for (int k = 0; k < PROF_POOL; ++k) {
        if (hipEventCreate(&c->ev0[k]) != hipSuccess || hipEventCreate(&c->ev1[k]) != hipSuccess)
            return fail(set_err(GK_ERR_HIP, "event create failed"));
    }
    if (hipStreamSynchronize(c->st) != hipSuccess) return fail(set_err(GK_ERR_HIP, "sync failed"));
    *out = c;
    return GK_OK;
}

int gk_destroy(gk_ctx *c) {
    if (c == nullptr) return GK_OK;
    (void)hipSetDevice(c->dev);
    if (c->broken && c->st) {
        // a broken context's stream may never drain: wait a bounded time, and leak the
        // context (rather than free memory its kernels may still touch) if it does not
        if (spin_until(c, query_stream, c->st, "destroy of a broken context") != GK_OK)
            return set_err(GK_ERR_COMM, "gk_destroy: the broken context's stream did not drain; its memory is kept");
    }
    if (c->st) (void)hipStreamSynchronize(c->st);
    graph_reset(c);
    mg_free(c);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->lev_a) (void)hipEventDestroy(c->lev_a);
    if (c->lev_b) (void)hipEventDestroy(c->lev_b);
    if (c->lscratch) (void)hipFree(c->lscratch);
    for (void *p : c->xs_mapped) (void)hipIpcCloseMemHandle(p);
    if (c->xs_buf) (void)hipFree(c->xs_buf);
    if (c->xs_seqdev) (void)hipFree(c->xs_seqdev);
    if (c->xs_err) (void)hipHostFree(c->xs_err);
    if (c->res_gath) (void)hipFree(c->res_gath);
    if (c->res_gm) (void)hipFree(c->res_gm);
    if (c->hold_word) (void)hipHostFree(c->hold_word);
    if (c->res_stamps) (void)hipFree(c->res_stamps);
    if (c->res_trace) (void)hipFree(c->res_trace);
    if (c->res_err) (void)hipHostFree(c->res_err);
    if (c->sr_dev) (void)hipFree(c->sr_dev);
    if (c->sr_mir) (void)hipHostFree(c->sr_mir);
    if (c->sr_hist) (void)hipFree(c->sr_hist);
    for (hipEvent_t e : c->sr_pend) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->sr_evfree) (void)hipEventDestroy(e);
    double *bufs[] = {c->V, c->w, c->z, c->aux, c->dA, c->dB, c->x, c->b, c->vj, c->hlo, c->hhi, c->dh, c->zline,
                      c->red, c->hcol, c->ydev, c->hb, c->scal, c->Vb, c->gram_slab, c->gram_out, c->cgs_slab, c->cgs_s};
    for (double *p : bufs)
        if (p) (void)hipFree(p);
    if (c->gram_pairs) (void)hipFree(c->gram_pairs);
    if (c->hcol_host) (void)hipHostFree(c->hcol_host);
    if (c->hall) (void)hipFree(c->hall);
    if (c->hallh) (void)hipHostFree(c->hallh);
    for (hipEvent_t e : c->ev_step)
        if (e) (void)hipEventDestroy(e);
    for (size_t k = 0; k < c->ev0.size(); ++k) {
        if (c->ev0[k]) (void)hipEventDestroy(c->ev0[k]);
        if (c->ev1[k]) (void)hipEventDestroy(c->ev1[k]);
    }
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
    return GK_OK;
}

int gk_local_size(gk_ctx *c, long long *nloc) {
    CHK(check_ctx(c));
    *nloc = c->nloc;
    return GK_OK;
}

int gk_set_precond(gk_ctx *c, int kind, const double *params, int nparams, int degree) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    if (kind < GK_PREC_IDENTITY || kind > GK_PREC_MG) return set_err(GK_ERR_ARG, "bad precond kind %d", kind);
    if (kind != GK_PREC_IDENTITY && (params == nullptr || nparams < 2))
        return set_err(GK_ERR_ARG, "precond needs params(1:2)");
    if (kind == GK_PREC_CHEB && (degree < 1 || degree > 64)) return set_err(GK_ERR_ARG, "bad degree %d", degree);
    if (kind == GK_PREC_MG) {  // everything checked, and the hierarchy built, before the context changes
        int sides[gk::MG_LMAX];
        if (gk::mg_levels(c->N, sides) < 2)
            return set_err(GK_ERR_ARG, "multigrid needs an even N with N / 2 >= %d (N = %d)", gk::MG_NMIN, c->N);
        if (degree < 1 || degree > gk::MG_DEG_MAX)
            return set_err(GK_ERR_ARG, "multigrid smoother degree %d outside 1..%d", degree, gk::MG_DEG_MAX);
        if (std::fabs(params[1] - params[0]) == 0.0) return set_err(GK_ERR_ARG, "multigrid smoother interval is empty");
        if (c->nranks > 1 || c->comm != nullptr || c->lg != nullptr || c->xs_on || c->line0 != 0 || c->nlines != c->N)
            return set_err(GK_ERR_STATE, "multigrid needs the whole grid on one rank (no communicator)");
        if (c->V == nullptr) return set_err(GK_ERR_ARG, "multigrid needs a context (gk_create)");
        HIPCHK(hipSetDevice(c->dev));
        // the same cycle again (the host-array plug-in sets it per application): keep the hierarchy
        const bool same = c->pkind == GK_PREC_MG && c->mg.size() >= 2 && c->p0 == params[0] && c->p1 == params[1] &&
                          c->pdeg == degree;
        if (!same) CHK(mg_build(c, params[0], params[1], degree));
    } else {
        mg_free(c);
    }
    c->pkind = kind;
    if (params != nullptr && nparams >= 2) {
        c->p0 = params[0];
        c->p1 = params[1];
    }
    c->pdeg = degree;
    graph_reset(c);
    if (kind == GK_PREC_CHEB && std::fabs(c->p1 - c->p0) == 0.0)
        return set_err(GK_ERR_ARG, "Chebyshev interval is empty");
    return GK_OK;
}

int gk_set_precond_side(gk_ctx *c, int side) {
    CHK(check_ctx(c));
    if (side != GK_SIDE_LEFT && side != GK_SIDE_RIGHT) return set_err(GK_ERR_ARG, "bad preconditioning side %d", side);
    sr_invalidate(c);
    c->cycle_mgs = c->cycle_hh = false;  // the open cycle's basis belongs to the other operator
    if (side != c->side) graph_reset(c);
    c->side = side;
    return GK_OK;
}

int gk_set_basis_precision(gk_ctx *c, int prec) {
    CHK(check_ctx(c));
    if (prec != GK_BASIS_F64 && prec != GK_BASIS_F32) return set_err(GK_ERR_ARG, "bad basis precision %d", prec);
    if (prec == GK_BASIS_F32) {
        if (c->nranks > 1 || c->comm != nullptr || c->lg != nullptr)
            return set_err(GK_ERR_STATE, "the FP32 basis needs a single-rank context (no communicator)");
        if (c->m < 3) return set_err(GK_ERR_ARG, "the FP32 basis needs m >= 3 (m = %d)", c->m);
        if (cgs_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis has no CGS2 step: set GK_ORTH_MGSR first");
    }
    sr_invalidate(c);
    c->cycle_mgs = c->cycle_hh = false;  // the open cycle's basis is stored in the other format
    if (prec != c->basis) graph_reset(c);  // the captured steps hold column pointers
    c->basis = prec;
    return GK_OK;
}

int gk_get_basis_precision(gk_ctx *c, int *prec) {
    CHK(check_ctx(c));
    if (prec == nullptr) return set_err(GK_ERR_ARG, "null prec");
    *prec = c->basis;
    return GK_OK;
}

int gk_set_orthogonalization(gk_ctx *c, int scheme) {
    CHK(check_ctx(c));
    if (scheme != GK_ORTH_MGSR && scheme != GK_ORTH_CGS2) return set_err(GK_ERR_ARG, "bad orthogonalization %d", scheme);
    if (scheme == GK_ORTH_CGS2 && cb_on(c))
        return set_err(GK_ERR_STATE, "the CGS2 step runs on FP64 columns: set GK_BASIS_F64 first");
    sr_invalidate(c);
    c->cycle_mgs = c->cycle_hh = false;  // the open cycle's columns were made by the other scheme
    if (scheme != c->orth) graph_reset(c);  // the captured steps are the other scheme's chains
    c->orth = scheme;
    return GK_OK;
}

int gk_get_orthogonalization(gk_ctx *c, int *scheme) {
    CHK(check_ctx(c));
    if (scheme == nullptr) return set_err(GK_ERR_ARG, "null scheme");
    *scheme = c->orth;
    return GK_OK;
}

int gk_cb_plan_query(long long nloc, int cus, int share, int m, long long *info) {
    if (info == nullptr || nloc < 2 || cus < 1 || share < 1 || m < 1) return set_err(GK_ERR_ARG, "bad plan query");
    static_assert(GK_CB_INFO_LEN == gk::CPI_LEN, "gk_cb_plan_query layout");
    gk::CbPlan p;
    gk::plan_cb(nloc, cus, share, m, p);
    gk::cb_plan_info(p, info);
    return GK_OK;
}

int gk_set_rhs(gk_ctx *c, const double *b) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->b, b, sizeof(double) * c->nloc, hipMemcpyHostToDevice, c->st));
    CHK(sync_st(c));
    c->beta0 = -1.0;
    return GK_OK;
}

int gk_set_rhs_ones(gk_ctx *c) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    HIPCHK(hipSetDevice(c->dev));
    gk::k_fill<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->aux, 1.0, c->nloc);
    LAUNCHCHK();
    CHK(op_A(c, c->aux, c->b, gk::ACC_NONE, nullptr, nullptr));
    CHK(sync_st(c));
    c->beta0 = -1.0;
    return GK_OK;
}

int gk_rhs_norm(gk_ctx *c, double *beta0) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    CHK(proj(c, gk::PJ_DOT, c->b, nullptr, c->b, nullptr, 0, slot(c, 0), nullptr, 1.0));
    CHK(allreduce(c, slot(c, 0), c->np_pj));
    CHK(finalize(c, slot(c, 0), c->np_pj, c->scal, 1));
    CHK(d2h_sync(c, beta0, c->scal, 1));
    c->beta0 = *beta0;
    return GK_OK;
}

int gk_zero_x(gk_ctx *c) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemsetAsync(c->x, 0, sizeof(double) * c->nloc, c->st));
    CHK(sync_st(c));
    return GK_OK;
}

int gk_get_x(gk_ctx *c, double *x) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(x, c->x, sizeof(double) * c->nloc, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    return GK_OK;
}

int gk_get_basis(gk_ctx *c, int which, int col, double *out) {
    CHK(check_ctx(c));
    const double *base = which == 0 ? c->V : (which == 1 ? c->Vb : nullptr);
    const int ncol = which == 0 ? c->m + 1 : c->m;
    if (base == nullptr) return set_err(GK_ERR_ARG, "basis %d not available", which);
    if (col < 0 || col >= ncol) return set_err(GK_ERR_ARG, "bad column %d", col);
    HIPCHK(hipSetDevice(c->dev));
    const double *src = base + (i64)col * c->ld;
    if (which == 0 && cb_on(c)) {  // the stored float column, widened (exact) through aux
        HIPCHK(gk::cb_widen(c->nblk_stream, c->aux, vcol<float>(c, col), c->nloc, c->st));
        src = c->aux;
    }
    HIPCHK(hipMemcpyAsync(out, src, sizeof(double) * c->nloc, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    return GK_OK;
}

// The inverse of gk_get_basis(which = 0).  FP32 basis: the values must be floats already
// (a second rounding here would hide the one under test); the column, and its widened
// copy in vjw (and in v1w when col == 0), exactly as k_scale_cb leaves them.
int gk_set_basis(gk_ctx *c, int col, const double *in) {
    CHK(check_ctx(c));
    if (in == nullptr) return set_err(GK_ERR_ARG, "null column");
    if (col < 0 || col > c->m) return set_err(GK_ERR_ARG, "bad column %d", col);
    std::vector<float> f;
    if (cb_on(c)) {
        f.resize((size_t)c->nloc);
        for (i64 e = 0; e < c->nloc; ++e) {
            // finite and within float's range first: converting a larger double is undefined
            const bool in_range = std::fabs(in[e]) <= (double)FLT_MAX;
            f[(size_t)e] = in_range ? (float)in[e] : 0.0f;
            if (!in_range || (double)f[(size_t)e] != in[e])
                return set_err(GK_ERR_ARG, "gk_set_basis: element %lld of column %d is not an FP32 value (FP32 basis)",
                               (long long)e, col);
        }
    }
    sr_invalidate(c);  // the short-recurrence vectors share the allocation
    HIPCHK(hipSetDevice(c->dev));
    const size_t nb = sizeof(double) * (size_t)c->nloc;
    if (cb_on(c)) {
        HIPCHK(hipMemcpyAsync(vcol<float>(c, col), f.data(), sizeof(float) * (size_t)c->nloc, hipMemcpyHostToDevice,
                              c->st));
        HIPCHK(hipMemcpyAsync(cb_vjw(c), in, nb, hipMemcpyHostToDevice, c->st));
        if (col == 0) HIPCHK(hipMemcpyAsync(cb_v1w(c), in, nb, hipMemcpyHostToDevice, c->st));
    } else {
        HIPCHK(hipMemcpyAsync(c->V + (i64)col * c->ld, in, nb, hipMemcpyHostToDevice, c->st));
    }
    CHK(sync_st(c));
    return GK_OK;
}

int gk_set_x(gk_ctx *c, const double *x) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->x, x, sizeof(double) * c->nloc, hipMemcpyHostToDevice, c->st));
    CHK(sync_st(c));
    return GK_OK;
}

int gk_true_residual(gk_ctx *c, double *rel) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    double b0;
    if (c->beta0 < 0) CHK(gk_rhs_norm(c, &b0));
    CHK(op_resid(c, c->x, c->aux, gk::ACC_NORM, slot(c, 2)));
    CHK(allreduce(c, slot(c, 2), c->np_st));
    CHK(finalize(c, slot(c, 2), c->np_st, c->scal + 1, 1));
    double r;
    CHK(d2h_sync(c, &r, c->scal + 1, 1));
    *rel = r / c->beta0;
    return GK_OK;
}

// ------------------------------------------------------------------ MGS-R --

int gk_mgs_cycle_start(gk_ctx *c, double *beta) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    HIPCHK(hipSetDevice(c->dev));
    if (c->pend_res_blk != 0 || c->pend_res_pf >= 0) {  // a step change requested mid-cycle (gk_set_tuning)
        if (c->pend_res_blk != 0) c->tune_res_blk = c->pend_res_blk;
        if (c->pend_res_pf >= 0) c->tune_res_pf = c->pend_res_pf;
        c->pend_res_blk = 0;
        c->pend_res_pf = -1;
        set_geometry(c);
        graph_reset(c);
    }
    if (right_prec(c))  // w = b - A x: the Arnoldi residual is the true residual
        CHK(op_resid(c, c->x, c->w, gk::ACC_NORM, slot(c, 0)));
    else
        CHK(op_precond(c, c->x, c->w, true, gk::ACC_NORM, nullptr, slot(c, 0)));
    CHK(allreduce(c, slot(c, 0), c->last_np));
    CHK(scale_col(c, 0, slot(c, 0), c->last_np, c->hcol));  // FP32 basis: also v1w and vjw, step 1's operands
    CHK(d2h_sync(c, beta, c->hcol, 1));
    c->cycle_mgs = true;
    c->cycle_hh = false;
    return GK_OK;
}

int gk_mgs_step_async(gk_ctx *c, int j) {
    CHK(check_ctx(c));
    if (j < 1 || j > c->m) return set_err(GK_ERR_ARG, "step j=%d outside 1..%d", j, c->m);
    if (!c->cycle_mgs) return set_err(GK_ERR_STATE, "gk_mgs_step before gk_mgs_cycle_start");
    HIPCHK(hipSetDevice(c->dev));
    const i64 ld = c->ld;
    double *V = c->V;
    const int m2 = c->m + 2;
    double *hs = c->hall + (i64)(j - 1) * m2;  // H(1:j+1, j) of this step, on device
    c->prof_on_step = (j % c->prof_every) == 0;
    const int s0 = 0;
    ResPlan rp;
    gk::CbPlan cp;
    const bool cb = cb_on(c);
    const bool cgs = cgs_on(c);  // its chain runs launch by launch (or as a graph): never a resident launch
    const bool res = cgs ? false : (cb ? cb_plan_ctx(c, cp) : res_plan(c, rp));
    if (cgs) CHK(ensure_cgs(c));
    // The CGS2 sweeps take every dot themselves: no fused first dot, except where the operator
    // route is chosen by it (Chebyshev on the left, op_precond_sten) -- its slab stays unconsumed.
    const int acc = cgs && !(c->pkind == GK_PREC_CHEB && !right_prec(c)) ? gk::ACC_NONE : gk::ACC_DOT;
    // the operator's input V(:,j) and the first dot's partner V(:,1); compressed basis: their
    // widened copies (the operator stage itself is the same launches)
    const double *vj = cb ? cb_vjw(c) : V + (i64)(j - 1) * ld, *v1 = cb ? cb_v1w(c) : V;
    // w = M^-1 A V(:,j) (side right: A M^-1 V(:,j)), fused with the first dot <w, V(:,1)>
    if (right_prec(c))
        CHK(op_right(c, vj, c->w, acc, v1, slot(c, s0)));
    else
        CHK(op_precond(c, vj, c->w, false, acc, v1, slot(c, s0)));
    int np = c->last_np;
    if (res) {  // the whole cascade + norm + scale as one resident launch
        // N ranks on the device exchange: the first dot's rank totals inside the launch
        // (GK_TUNE_RES_FOLD) instead of a k_xchg launch before it
        const bool fold = c->tune_res_fold && c->xs_on && c->nranks > 1;
        if (!fold) CHK(allreduce(c, slot(c, s0), np));
        if (cb)  // ... on float columns (k_mgs_wcb; one rank)
            CHK(cb_step(c, j, cp, slot(c, s0), np, hs, c->hallh_dev + (i64)(j - 1) * m2));
        else
            CHK(res_step(c, j, rp, slot(c, s0), np, hs, c->hallh_dev + (i64)(j - 1) * m2, gk::RES_MGS, nullptr, -1,
                         fold ? RESF_PIN_LOCAL : 0));
        HIPCHK(hipEventRecord(c->ev_step[j], c->st));
        c->prof_on_step = true;
        return GK_OK;
    }
    // Launch path: RCCL ranks (or one rank with the resident step off) replay the
    // step's projection chain as a hipGraph captured at its first use (GK_TUNE_GRAPH).
    if (c->tune_graph && (c->lg == nullptr || c->xs_on)) {
        if (c->gkey != np) {
            graph_reset(c);
            c->gkey = np;
        }
        if ((int)c->gstep.size() < c->m + 1) c->gstep.resize(c->m + 1, nullptr);
        if (c->gstep[j] == nullptr) CHK(capture_step(c, j, np));
        if (c->gstep[j] != nullptr) {
            {
                ProfScope ps(c, GK_KID_GRAPH);
                if (c->xs_on && c->gxs[j] > 0) {  // the replay's exchanges continue this context's numbering
                    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->xs_seqdev), (int)c->xs_seq, 1, c->st));
                    c->xs_seq += c->gxs[j];
                }
                HIPCHK(hipGraphLaunch(c->gstep[j], c->st));
            }
            HIPCHK(hipEventRecord(c->ev_step[j], c->st));
            c->prof_on_step = true;
            return GK_OK;
        }
    }
    CHK(mgs_chain(c, j, np));
    HIPCHK(hipEventRecord(c->ev_step[j], c->st));
    c->prof_on_step = true;
    return GK_OK;
}

// The host's per-step wait for the Hessenberg column.  Spinning on the event
// (default) keeps the wake-up off the critical path: a blocking wait sleeps
// in the driver and costs a scheduler wake-up per Arnoldi step, which a
// process that initialised another HIP user first (torch) was measured to
// pay -- 1024^2 cycles 37.0 -> 45.8 ms with identical kernel times.
int wait_step_event(gk_ctx *c, hipEvent_t e) {
    if (!c->tune_spin_wait) {
        HIPCHK(hipEventSynchronize(e));
        return GK_OK;
    }
    return spin_until(c, query_event, e, "Arnoldi step wait");
}

int gk_mgs_step_wait(gk_ctx *c, int j, double *hcol) {
    CHK(check_ctx(c));
    if (j < 1 || j > c->m) return set_err(GK_ERR_ARG, "step j=%d outside 1..%d", j, c->m);
    CHK(wait_step_event(c, c->ev_step[j]));
    CHK(res_check(c));
    CHK(xs_check(c));
    const volatile double *src = c->hallh + (i64)(j - 1) * (c->m + 2);
    for (int k = 0; k <= j; ++k) hcol[k] = src[k];
    return GK_OK;
}

int gk_mgs_step(gk_ctx *c, int j, double *hcol) {
    CHK(gk_mgs_step_async(c, j));
    return gk_mgs_step_wait(c, j, hcol);
}

int gk_update_x(gk_ctx *c, const double *y, int n_out) {
    CHK(check_ctx(c));
    if (n_out < 1 || n_out > c->m) return set_err(GK_ERR_ARG, "bad n_out %d", n_out);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->ydev, y, sizeof(double) * n_out, hipMemcpyHostToDevice, c->st));
    if (right_prec(c)) {  // x += M^-1 (V y): t = V y in w, M^-1 t in z
        CHK(update_x<false>(c, c->w, n_out));
        CHK(add_precond_sweeps(c, c->w));
    } else {
        CHK(update_x<true>(c, c->x, n_out));
    }
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    return GK_OK;
}

int gk_mgs_verr(gk_ctx *c, int n_out, int zero_last, double *v_err) {
    CHK(check_ctx(c));
    if (n_out < 1 || n_out > c->m) return set_err(GK_ERR_ARG, "bad n_out %d", n_out);
    HIPCHK(hipSetDevice(c->dev));
    const int nc = n_out + 1;
    std::vector<double> G;
    CHK(gram(c, c->V, nc, G));
    if (zero_last)
        for (int i = 0; i < nc; ++i) {
            G[(size_t)(nc - 1) * nc + i] = 0.0;
            G[(size_t)i * nc + nc - 1] = 0.0;
        }
    // v_err(j+1) = sqrt(v_err(j)^2 + sum_{i<=j} 2 (V_i.V_{j+1})^2 + (V_{j+1}.V_{j+1}-1)^2)
    for (int k = 0; k <= c->m; ++k) v_err[k] = 0.0;
    for (int j = 1; j <= n_out; ++j) {
        double s = 0.0;
        for (int i = 1; i <= j; ++i) {
            const double d = G[(size_t)j * nc + (i - 1)];
            s = s + 2.0 * (d * d);
        }
        const double dd = G[(size_t)j * nc + j] - 1.0;
        s = s + dd * dd;
        v_err[j] = std::sqrt(v_err[j - 1] * v_err[j - 1] + s);
    }
    return GK_OK;
}

// ------------------------------------------------------------- Householder --

// GK_TUNE_HH_NORM_ORDER: the reflector norms in flang-rt's order -- a running sum over
// the whole vector, so one rank only (N ranks keep the tree).
static bool hh_seq_norms(const gk_ctx *c) { return c->tune_hh_norm_order != 0 && c->nranks == 1; }

// The `precondition` argument of a cycle start or a step: one of GK_HH_PREC_*, and the left
// side only where the context's MGS-R side is left too (GK_HH_PREC_RIGHT asks for its side itself).
static int hh_prec_arg(const gk_ctx *c, int precondition) {
    if (precondition != GK_HH_PREC_NONE && precondition != GK_HH_PREC_LEFT && precondition != GK_HH_PREC_RIGHT)
        return set_err(GK_ERR_ARG, "precondition = %d is none of GK_HH_PREC_NONE / _LEFT / _RIGHT", precondition);
    if (precondition == GK_HH_PREC_LEFT && right_prec(c))
        return set_err(GK_ERR_STATE, "precondition = GK_HH_PREC_LEFT preconditions on the left only: "
                                     "gk_set_precond_side(ctx, GK_SIDE_LEFT) first, or GK_HH_PREC_RIGHT");
    return GK_OK;
}

static int hh_pivot(gk_ctx *c, int j) {
    // hb[0..j] = w(1:j+1) from the owning rank, broadcast
    const int root = owner_of(c, j);
    if (c->rank == root)
        HIPCHK(hipMemcpyAsync(c->hb, c->w + (0 - c->g0), sizeof(double) * (j + 1), hipMemcpyDeviceToDevice, c->st));
    return bcast(c, c->hb, j + 1, root);
}

int gk_hh_cycle_start(gk_ctx *c, int precondition, double *g1) {
    CHK(check_ctx(c));
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis is MGS-R only (gk_set_basis_precision)");
    sr_invalidate(c);
    HIPCHK(hipSetDevice(c->dev));
    if (c->nranks > 1 && c->rank == 0 && c->nloc < c->m + 2)
        return set_err(GK_ERR_ARG, "Householder path needs the first slab to hold m+2 unknowns");
    CHK(hh_prec_arg(c, precondition));
    if (precondition == GK_HH_PREC_LEFT)
        CHK(op_precond(c, c->x, c->w, true, gk::ACC_NORM, nullptr, slot(c, 0)));
    else  // none, or right: the Arnoldi residual is the true residual b - A x
        CHK(op_resid(c, c->x, c->w, gk::ACC_NORM, slot(c, 0)));
    CHK(allreduce(c, slot(c, 0), c->last_np));
    // GK_TUNE_HH_NORM_ORDER: beta = norm2(w) and norm2 of the fixed w in the reference's
    // order (gmres_hh.f90:250-253), one rank
    const bool seq = hh_seq_norms(c);
    if (seq) CHK(norm2_seq(c, c->w, c->nloc, slot(c, 0)));
    CHK(hh_pivot(c, 0));
    {
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_hh_pivot<<<1, gk::TPB, 0, c->st>>>(c->hb, slot(c, 0), seq ? 1 : c->last_np, 0, c->hcol, c->scal + 2,
                                                 nullptr, seq ? 1 : 0);
        LAUNCHCHK();
        // w(1) = sign(beta,w(1)) + w(1); norm2(w)
        gk::k_hh_fix<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->w, c->nloc, c->g0, 0, 0, c->scal + 2, slot(c, 1));
        LAUNCHCHK();
    }
    if (seq) {
        CHK(norm2_seq(c, c->w, c->nloc, slot(c, 1)));
        CHK(scale(c, c->V, c->w, slot(c, 1), 1, nullptr, nullptr, nullptr, 0, true));
    } else {
        CHK(allreduce(c, slot(c, 1), c->nblk_stream));
        CHK(scale(c, c->V, c->w, slot(c, 1), c->nblk_stream, nullptr));
    }
    CHK(d2h_sync(c, g1, c->hcol, 1));
    c->cycle_hh = true;
    c->cycle_mgs = false;
    c->hh_prec = precondition;
    return GK_OK;
}

int gk_hh_step_async(gk_ctx *c, int j, int precondition) {
    CHK(check_ctx(c));
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis is MGS-R only (gk_set_basis_precision)");
    if (j < 1 || j > c->m) return set_err(GK_ERR_ARG, "step j=%d outside 1..%d", j, c->m);
    if (!c->cycle_hh) return set_err(GK_ERR_STATE, "gk_hh_step before gk_hh_cycle_start");
    CHK(hh_prec_arg(c, precondition));
    if ((precondition == GK_HH_PREC_RIGHT) != (c->hh_prec == GK_HH_PREC_RIGHT))
        return set_err(GK_ERR_STATE, "gk_hh_step with precondition = %d in a cycle started with %d", precondition,
                       c->hh_prec);
    HIPCHK(hipSetDevice(c->dev));
    const i64 ld = c->ld;
    double *P = c->V;
    // The w-only resident variant folds the step's small launches into its chains
    // (GK_TUNE_HH_FUSE): the DOWN chain builds e_j itself (no k_set_unit), the UP
    // chain ends with the fix-up and P(:,j+1) = w/||w|| (no k_hh_fix, no k_scale).
    ResPlan rp;
    const bool res = res_plan(c, rp, true);
    const bool seq = hh_seq_norms(c);  // reference-order reflector norms: the unfused step
    const bool fuse = res && rp.wo && c->tune_hh_fuse != 0 && !seq;
    // v_j = e_j ; v_j = P_1 .. P_j e_j
    if (!fuse) {
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_set_unit<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->vj, c->nloc, c->g0, j - 1, 1.0);
        LAUNCHCHK();
    }
    CHK(reflect_chain_down(c, c->vj, j, j - 1, fuse ? RESF_UNIT_INIT : 0));
    // w = M^-1 A v_j (right: A M^-1 v_j; none, or the identity on the right: A v_j), fused with <w, P_1>
    int s0 = 0, s1 = 1;
    if (precondition == GK_HH_PREC_LEFT) {
        CHK(op_precond(c, c->vj, c->w, false, gk::ACC_DOT, P, slot(c, s0)));
    } else if (precondition == GK_HH_PREC_RIGHT && c->pkind != GK_PREC_IDENTITY) {
        CHK(op_right(c, c->vj, c->w, gk::ACC_DOT, P, slot(c, s0)));
    } else {
        CHK(op_A(c, c->vj, c->w, gk::ACC_DOT, P, slot(c, s0)));
    }
    int np = c->last_np;
    // N ranks on the device exchange: <w, P_1> summed across ranks inside the launch (GK_TUNE_RES_FOLD)
    const bool fold = res && c->tune_res_fold && c->xs_on && c->nranks > 1;
    if (fuse) {  // w = P_j .. P_1 w, ||w(j+1:n)||^2, the fix-up and P(:,j+1), one launch
        if (!fold) CHK(allreduce(c, slot(c, s0), np));
        CHK(res_step(c, j, rp, slot(c, s0), np, slot(c, s1), nullptr, gk::RES_HH_UP, c->w, -1,
                     RESF_CLOSE_HH | (fold ? RESF_PIN_LOCAL : 0)));
        // H(1:j+1, j) from hb (written by the owner rank's launch) on every rank
        CHK(bcast(c, c->hb, j + 1, owner_of(c, j)));
        {
            ProfScope ps(c, GK_KID_OTHER);
            const int m2 = c->m + 2;
            gk::k_hh_pivot<<<1, gk::TPB, 0, c->st>>>(c->hb, slot(c, s1), 1, j, c->hall + (i64)(j - 1) * m2,
                                                     c->scal + 2, c->hallh_dev + (i64)(j - 1) * m2);
            LAUNCHCHK();
        }
        HIPCHK(hipEventRecord(c->ev_step[j], c->st));
        return GK_OK;
    }
    if (res) {  // w = P_j .. P_1 w and ||w(j+1:n)||^2 as one resident launch
        if (!fold) CHK(allreduce(c, slot(c, s0), np));
        CHK(res_step(c, j, rp, slot(c, s0), np, slot(c, s1), nullptr, gk::RES_HH_UP, c->w, -1,
                     fold ? RESF_PIN_LOCAL : 0));
        std::swap(s0, s1);
        np = 1;  // slot s0[0]: the rank-summed total
    } else {
        // w = P_j .. P_1 w ; the last reflection also accumulates ||w(j+1:n)||^2
        for (int i = 1; i <= j; ++i) {
            CHK(allreduce(c, slot(c, s0), np));
            const double *va = P + (i64)(i - 1) * ld;
            if (i < j) {
                CHK(proj(c, gk::PJ_AXPY_DOT, c->w, va, P + (i64)i * ld, slot(c, s0), np, slot(c, s1), nullptr,
                         2.0));
            } else {
                CHK(proj(c, gk::PJ_AXPY_NORM, c->w, va, nullptr, slot(c, s0), np, slot(c, s1), nullptr, 2.0,
                         (i64)j - c->g0));
            }
            np = c->np_pj;
            std::swap(s0, s1);
        }
        CHK(allreduce(c, slot(c, s0), np));
    }
    if (seq) {  // tmp = norm2(w(j+1:n)) in the reference's order (gmres_hh.f90:307)
        CHK(norm2_seq(c, c->w + j, c->nloc - j, slot(c, s0)));
        np = 1;
    }
    CHK(hh_pivot(c, j));
    {
        ProfScope ps(c, GK_KID_OTHER);
        const int m2 = c->m + 2;
        gk::k_hh_pivot<<<1, gk::TPB, 0, c->st>>>(c->hb, slot(c, s0), np, j, c->hall + (i64)(j - 1) * m2,
                                                 c->scal + 2, c->hallh_dev + (i64)(j - 1) * m2, seq ? 1 : 0);
        LAUNCHCHK();
        gk::k_hh_fix<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->w, c->nloc, c->g0, j, j, c->scal + 2, slot(c, s1));
        LAUNCHCHK();
    }
    if (seq) {  // w = w / norm2(w) (gmres_hh.f90:315)
        CHK(norm2_seq(c, c->w, c->nloc, slot(c, s1)));
        CHK(scale(c, P + (i64)j * ld, c->w, slot(c, s1), 1, nullptr, nullptr, nullptr, 0, true));
    } else {
        CHK(allreduce(c, slot(c, s1), c->nblk_stream));
        CHK(scale(c, P + (i64)j * ld, c->w, slot(c, s1), c->nblk_stream, nullptr));
    }
    HIPCHK(hipEventRecord(c->ev_step[j], c->st));
    return GK_OK;
}

int gk_hh_step_wait(gk_ctx *c, int j, double *hcol) {
    return gk_mgs_step_wait(c, j, hcol);  // same per-step slot + event protocol
}

int gk_hh_step(gk_ctx *c, int j, int precondition, double *hcol) {
    CHK(gk_hh_step_async(c, j, precondition));
    return gk_hh_step_wait(c, j, hcol);
}

int gk_hh_update_x(gk_ctx *c, const double *y, int n_out) {
    CHK(check_ctx(c));
    if (n_out < 1 || n_out > c->m) return set_err(GK_ERR_ARG, "bad n_out %d", n_out);
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->ydev, y, sizeof(double) * n_out, hipMemcpyHostToDevice, c->st));
    {
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_set_prefix<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->w, c->nloc, c->g0, c->ydev, 0, n_out);
        LAUNCHCHK();
    }
    CHK(reflect_chain_down(c, c->w, n_out));
    if (c->hh_prec == GK_HH_PREC_RIGHT && c->pkind != GK_PREC_IDENTITY) {  // x += M^-1 t, t in w
        CHK(add_precond(c, c->w));
    } else {
        CHK(add_into(c, c->x, c->w));
    }
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    return GK_OK;
}

int gk_hh_verr(gk_ctx *c, int n_out, double *v_err) {
    CHK(check_ctx(c));
    if (n_out < 1 || n_out > c->m) return set_err(GK_ERR_ARG, "bad n_out %d", n_out);
    HIPCHK(hipSetDevice(c->dev));
    if (c->Vb == nullptr) {
        if (hipMalloc(&c->Vb, sizeof(double) * (size_t)c->ld * c->m) != hipSuccess)
            return set_err(GK_ERR_NOMEM, "cannot allocate the verr basis");
    }
    for (int i = 1; i <= n_out; ++i) {
        double *col = c->Vb + (i64)(i - 1) * c->ld;
        gk::k_set_unit<<<c->nblk_stream, gk::TPB, 0, c->st>>>(col, c->nloc, c->g0, i - 1, 1.0);
        LAUNCHCHK();
        if (!verr_ref_order(c)) CHK(reflect_chain_down(c, col, i, i - 1));
    }
    if (verr_ref_order(c)) {  // :581-585 with the reference's dots, all chains level by level
        CHK(ensure_gram(c, n_out));
        ProfScope ps(c, GK_KID_OTHER);
        for (int s = 0; s < n_out; ++s) {
            gk::k_hh_rebuild_dot<<<(n_out - s + 63) / 64, 64, 0, c->st>>>(c->Vb, c->V, c->ld, c->nloc, s, n_out,
                                                                          c->gram_out);
            LAUNCHCHK();
            gk::k_hh_rebuild_upd<<<dim3(c->nblk_stream, n_out - s), gk::TPB, 0, c->st>>>(c->Vb, c->V, c->ld,
                                                                                       c->nloc, s, c->gram_out);
            LAUNCHCHK();
        }
    }
    std::vector<double> G;
    CHK(gram(c, c->Vb, n_out, G));
    for (int k = 0; k <= c->m; ++k) v_err[k] = 0.0;
    for (int i = 2; i <= n_out; ++i) {
        double s = 0.0;
        for (int jj = 1; jj < i; ++jj) {
            const double d = G[(size_t)(i - 1) * n_out + (jj - 1)];
            s = s + 2.0 * (d * d);
        }
        v_err[i - 1] = s;
    }
    return GK_OK;
}

int gk_apply(gk_ctx *c, int what, const double *in, double *out) {
    CHK(check_ctx(c));
    if (in == nullptr || out == nullptr || (what != 0 && what != 1)) return set_err(GK_ERR_ARG, "bad gk_apply args");
    HIPCHK(hipSetDevice(c->dev));
    c->cycle_mgs = c->cycle_hh = false;  // clobbers the work vectors
    if (what == 0) {
        HIPCHK(hipMemcpyAsync(c->vj, in, sizeof(double) * c->nloc, hipMemcpyHostToDevice, c->st));
        CHK(op_A(c, c->vj, c->w, gk::ACC_NONE, nullptr, nullptr));
    } else {
        HIPCHK(hipMemcpyAsync(c->z, in, sizeof(double) * c->nloc, hipMemcpyHostToDevice, c->st));
        CHK(op_Minv_or_copy(c, c->z, c->w));
    }
    HIPCHK(hipMemcpyAsync(out, c->w, sizeof(double) * c->nloc, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    return GK_OK;
}

int gk_set_tuning(gk_ctx *c, int key, int value) {
    CHK(check_ctx(c));
    switch (key) {
        case GK_TUNE_PROJ_NT: c->tune_nt = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_PROJ_BLOCKS: c->tune_pj_blocks = value; break;
        case GK_TUNE_STENCIL_BLOCKS: c->tune_st_blocks = value; break;
        case GK_TUNE_CHEB_FUSED: c->tune_cheb_fused = value != 0; break;
        case GK_TUNE_XCHG_TIMEOUT_MS:
            if (value < 1) return set_err(GK_ERR_ARG, "timeout must be >= 1 ms");
            xs_set_timeout(c, value);
            break;
        case GK_TUNE_RES: c->tune_res = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_RES_R2:
            if (value != 0 && value != 2 && value != 4 && value != 8 && value != 12)
                return set_err(GK_ERR_ARG, "resident cap must be 0 (auto), 2, 4, 8 or 12");
            c->tune_res_r2 = value;
            break;
        case GK_TUNE_RES_SHARE:
            if (value < 1) return set_err(GK_ERR_ARG, "share must be >= 1");
            c->res_share = value;
            break;
        case GK_TUNE_RES_WONLY: c->tune_res_wonly = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_RES_PIPE: c->tune_res_pipe = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_RES_PIPE_CARRY: c->tune_res_carry = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_HH_FUSE: c->tune_hh_fuse = value != 0; break;
        case GK_TUNE_CHEB_STEN: c->tune_cheb_sten = value != 0; break;
        case GK_TUNE_SPIN_WAIT: c->tune_spin_wait = value != 0; break;
        case GK_TUNE_GRAPH: c->tune_graph = value != 0; break;
        case GK_TUNE_RES_QDEF: c->tune_res_qdef = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_RES_PC: c->tune_res_pc = value < 0 ? -1 : (value != 0); break;
        case GK_TUNE_RES_FOLD: c->tune_res_fold = value != 0; break;
        case GK_TUNE_WATCHDOG_MS: c->watchdog_ms = std::max(0, value); break;
        case GK_TUNE_HH_NORM_ORDER: c->tune_hh_norm_order = value != 0; break;
        // The blocked step reads Gram rows of earlier columns that only a blocked step of the
        // same cycle wrote: switching the step inside a cycle would use stale rows, so a change
        // requested while a cycle is open takes effect at the next gk_mgs_cycle_start.
        case GK_TUNE_RES_BLOCK:
            if (value != 1 && value != 2 && value != 4)
                return set_err(GK_ERR_ARG, "GK_TUNE_RES_BLOCK %d: blocks of 1 (strict MGS-R), 2 or 4 projections", value);
            if (c->cycle_mgs)
                c->pend_res_blk = value;
            else
                c->tune_res_blk = value;
            break;
        case GK_TUNE_SR_BLOCKS: c->tune_sr_blocks = std::max(0, value); break;
        case GK_TUNE_SR_TWO_LEVEL: c->tune_sr_two = value != 0; break;
        case GK_TUNE_RES_PF:
            if (c->cycle_mgs)
                c->pend_res_pf = value != 0;
            else
                c->tune_res_pf = value != 0;
            break;
        case GK_TUNE_VERR_ORDER: c->tune_verr_order = value != 0; break;
        case GK_TUNE_RIGHT_FUSED: c->tune_right_fused = value != 0; break;
        case GK_TUNE_MG_FUSED: c->tune_mg_fused = value != 0; break;
        case GK_TUNE_RES_TIMEOUT_MS:
            if (value < 1) return set_err(GK_ERR_ARG, "timeout must be >= 1 ms");
            c->res_timeout_ms = value;
            break;
        default: return set_err(GK_ERR_ARG, "unknown tuning key %d", key);
    }
    set_geometry(c);
    graph_reset(c);
    return GK_OK;
}

// ---------------------------------------------------------------- profiling --

int gk_profile_enable(gk_ctx *c, int enable) {
    CHK(check_ctx(c));
    if (!enable) CHK(prof_harvest(c));
    c->prof = enable != 0;
    c->prof_every = enable > 1 ? enable : 1;
    c->prof_on_step = true;
    return GK_OK;
}

int gk_profile_reset(gk_ctx *c) {
    CHK(check_ctx(c));
    CHK(prof_harvest(c));
    for (int k = 0; k < GK_NKID; ++k) {
        c->prof_ms[k] = 0.0;
        c->prof_n[k] = 0;
    }
    return GK_OK;
}

int gk_profile_read(gk_ctx *c, int kid, double *total_ms, long long *launches) {
    CHK(check_ctx(c));
    if (kid < 0 || kid >= GK_NKID) return set_err(GK_ERR_ARG, "bad kernel id");
    CHK(prof_harvest(c));
    *total_ms = c->prof_ms[kid];
    *launches = c->prof_n[kid];
    return GK_OK;
}

int gk_profile_res_wg(gk_ctx *c, int which, double *pass_ms, double *wait_ms, int maxwg, int *nwg) {
    CHK(check_ctx(c));
    if (which < 0 || which > 2 || pass_ms == nullptr || wait_ms == nullptr || nwg == nullptr || maxwg < 1)
        return set_err(GK_ERR_ARG, "bad arguments");
    *nwg = 0;
    if (c->res_stamps == nullptr) return GK_OK;
    HIPCHK(hipSetDevice(c->dev));
    std::vector<gk::u64> h(4 * (size_t)gk::RGMAX);
    HIPCHK(hipMemcpyAsync(h.data(), c->res_stamps + (size_t)which * 4 * gk::RGMAX, sizeof(gk::u64) * h.size(),
                          hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    const double tpm = (double)c->xs_tick_per_ms;
    int g = 0;
    for (int b = 0; b < gk::RGMAX && g < maxwg; ++b)
        if (h[4 * b + 3] > 0) {  // workgroups that ran, in blockIdx order
            pass_ms[g] = (double)h[4 * b] / tpm;
            wait_ms[g] = (double)h[4 * b + 1] / tpm;
            ++g;
        }
    *nwg = g;
    return GK_OK;
}

int gk_profile_res_trace(gk_ctx *c, int arm, int j, int mode, unsigned long long *out, int maxwg, int maxx,
                         int *nwg, int *nx, double *tick_per_ms) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    const size_t words = (size_t)gk::RGMAX * gk::RES_TRACE_X * 2;
    if (arm == 1) {
        if (mode != gk::RES_MGS || j < 1) return set_err(GK_ERR_ARG, "trace: MGS-R step launches (mode 0), j >= 1");
        if (c->res_trace == nullptr) HIPCHK(hipMalloc(&c->res_trace, sizeof(gk::u64) * words));
        HIPCHK(hipMemsetAsync(c->res_trace, 0, sizeof(gk::u64) * words, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        c->res_trace_j = j;
        c->res_trace_mode = mode;
        c->res_trace_g = c->res_trace_np = 0;
        return GK_OK;
    }
    if (arm == 0) {
        c->res_trace_mode = -1;
        return GK_OK;
    }
    if (out == nullptr || nwg == nullptr || nx == nullptr || tick_per_ms == nullptr || maxwg < 1 || maxx < 1)
        return set_err(GK_ERR_ARG, "bad arguments");
    *nwg = *nx = 0;
    *tick_per_ms = (double)c->xs_tick_per_ms;
    if (c->res_trace == nullptr || c->res_trace_g == 0) return GK_OK;
    std::vector<gk::u64> h(words);
    HIPCHK(hipMemcpyAsync(h.data(), c->res_trace, sizeof(gk::u64) * words, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    const int G = std::min(c->res_trace_g, maxwg), X = std::min({c->res_trace_np, maxx, gk::RES_TRACE_X});
    for (int b = 0; b < G; ++b)
        for (int x = 0; x < X; ++x)
            for (int k = 0; k < 2; ++k)
                out[((size_t)b * X + x) * 2 + k] = h[((size_t)b * gk::RES_TRACE_X + x) * 2 + k];
    *nwg = G;
    *nx = X;
    return GK_OK;
}

int gk_profile_res_split(gk_ctx *c, int mode, int which, double *pass_ms, double *wait_ms, double *total_ms,
                         long long *launches) {
    CHK(check_ctx(c));
    if (which < 0 || which > 2) return set_err(GK_ERR_ARG, "which must be 0 (MGS), 1 (HH up) or 2 (HH down)");
    HIPCHK(hipSetDevice(c->dev));
    const size_t bytes = sizeof(gk::u64) * 4 * 3 * gk::RGMAX;
    if (mode == 1 || mode == 2) {  // enable (and zero) / reset
        if (c->res_stamps == nullptr) HIPCHK(hipMalloc(&c->res_stamps, bytes));
        HIPCHK(hipMemsetAsync(c->res_stamps, 0, bytes, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        c->res_split = true;
    } else if (mode == 0) {
        c->res_split = false;
    }
    if (pass_ms == nullptr || wait_ms == nullptr || total_ms == nullptr || launches == nullptr) return GK_OK;
    *pass_ms = *wait_ms = *total_ms = 0.0;
    *launches = 0;
    if (c->res_stamps == nullptr) return GK_OK;
    std::vector<gk::u64> h(4 * (size_t)gk::RGMAX);
    HIPCHK(hipMemcpyAsync(h.data(), c->res_stamps + (size_t)which * 4 * gk::RGMAX, sizeof(gk::u64) * h.size(),
                          hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    // mean over the workgroups that ran (slot launches > 0), in ms of wall clock
    double sp = 0, sw = 0, st = 0;
    int g = 0;
    long long nl = 0;
    for (int b = 0; b < gk::RGMAX; ++b)
        if (h[4 * b + 3] > 0) {
            sp += (double)h[4 * b];
            sw += (double)h[4 * b + 1];
            st += (double)h[4 * b + 2];
            nl = std::max<long long>(nl, (long long)h[4 * b + 3]);
            ++g;
        }
    if (g > 0) {
        const double tpm = (double)c->xs_tick_per_ms;
        *pass_ms = sp / g / tpm;
        *wait_ms = sw / g / tpm;
        *total_ms = st / g / tpm;
    }
    *launches = nl;
    return GK_OK;
}

int gk_debug_hold_stream(gk_ctx *c, int hold) {
    if (c == nullptr) return set_err(GK_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->dev));
    if (c->hold_word == nullptr) {
        HIPCHK(hipHostMalloc((void **)&c->hold_word, sizeof(unsigned), hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer((void **)&c->hold_word_dev, c->hold_word, 0));
        *c->hold_word = 0;
    }
    if (hold) {
        if (c->broken) return set_err(GK_ERR_STATE, "context broken");
        __atomic_store_n(c->hold_word, 0u, __ATOMIC_RELEASE);
        HIPCHK(hipStreamWaitValue32(c->st, c->hold_word_dev, 1u, hipStreamWaitValueGte, 0xFFFFFFFFu));
    } else {
        __atomic_store_n(c->hold_word, 1u, __ATOMIC_RELEASE);
    }
    return GK_OK;
}

int gk_sync(gk_ctx *c) {
    CHK(check_ctx(c));
    HIPCHK(hipSetDevice(c->dev));
    CHK(sync_st(c));
    if (c->prof) CHK(prof_harvest(c));
    return GK_OK;
}

int gk_res_plan_query(long long nloc, int cus, int share, int hh, int nt, int block, long long *info) {
    if (info == nullptr || nloc < 2 || cus < 1 || share < 1 || (block != 1 && block != 2 && block != 4))
        return set_err(GK_ERR_ARG, "bad plan query");
    const int gmax = std::max(1, std::min(gk::RGMAX, cus / share));
    ResPlan p;
    plan_resident(nloc, gmax, RES_R2_BIG, -1, hh != 0, nt < 0 ? nt_auto_for(nloc) : nt != 0, p, -1, block);
    plan_info(p, true, info);
    return GK_OK;
}

// info: [0] levels, [1] the coarsest level's sweep count, [2] the smoother degree (0 from the
// plan query), [3 ..] the level sides
static void mg_info_fill(const int *sides, int nl, int cdeg, int deg, int *info) {
    for (int k = 0; k < GK_MG_INFO_LEN; ++k) info[k] = 0;
    info[0] = nl;
    info[1] = cdeg;
    info[2] = deg;
    for (int l = 0; l < nl && 3 + l < GK_MG_INFO_LEN; ++l) info[3 + l] = sides[l];
}

int gk_mg_plan_query(int nside, int *info) {
    static_assert(GK_MG_INFO_LEN >= 3 + gk::MG_LMAX, "gk_mg_plan_query layout");
    if (info == nullptr) return set_err(GK_ERR_ARG, "null info");
    int sides[gk::MG_LMAX];
    const int nl = gk::mg_levels(nside, sides);
    if (nl < 2) return set_err(GK_ERR_ARG, "multigrid needs an even N with N / 2 >= %d (N = %d)", gk::MG_NMIN, nside);
    double lo, hi;
    mg_info_fill(sides, nl, gk::mg_coarse_degree(sides[nl - 1], &lo, &hi), 0, info);
    return GK_OK;
}

int gk_mg_info(gk_ctx *c, int *info) {
    CHK(check_ctx(c));
    if (info == nullptr) return set_err(GK_ERR_ARG, "null info");
    if (c->pkind != GK_PREC_MG || c->mg.size() < 2) return set_err(GK_ERR_STATE, "no multigrid preconditioner set");
    int sides[gk::MG_LMAX];
    const int nl = (int)c->mg.size();
    for (int l = 0; l < nl; ++l) sides[l] = c->mg[l].lc->N;
    mg_info_fill(sides, nl, c->mg_cdeg, c->pdeg, info);
    return GK_OK;
}

int gk_mg_transfer(gk_ctx *c, int what, int level, const double *a, const double *b, double *out) {
    CHK(check_ctx(c));
    if (c->pkind != GK_PREC_MG || c->mg.size() < 2) return set_err(GK_ERR_STATE, "no multigrid preconditioner set");
    if (what < 0 || what > 2 || level < 0 || level + 1 >= (int)c->mg.size() || a == nullptr || out == nullptr ||
        (what != 0 && b == nullptr))
        return set_err(GK_ERR_ARG, "bad gk_mg_transfer(%d, level %d)", what, level);
    HIPCHK(hipSetDevice(c->dev));
    c->cycle_mgs = c->cycle_hh = false;  // clobbers the hierarchy's work vectors
    sr_invalidate(c);
    return mg_transfer(c, what, level, a, b, out);
}

int gk_res_info(gk_ctx *c, int hh, long long *info) {
    CHK(check_ctx(c));
    if (info == nullptr) return set_err(GK_ERR_ARG, "null info");
    ResPlan p;
    const bool on = !(hh == 0 && cgs_on(c)) && res_plan(c, p, hh != 0);  // a CGS2 context's MGS step: launch by launch
    plan_info(p, on, info);
    if (cb_on(c) && hh == 0) {  // the MGS-R step of a compressed-basis context: k_mgs_wcb's plan
        gk::CbPlan cp;
        const bool cbon = cb_plan_ctx(c, cp);
        for (int k = 0; k < GK_RES_INFO_LEN; ++k) info[k] = 0;
        if (cbon) {
            info[gk::RPI_VARIANT] = GK_RES_CB;
            info[gk::RPI_G] = cp.G;
            info[gk::RPI_R2] = gk::CB_RW;
            info[gk::RPI_L2] = gk::CB_LW;
            info[gk::RPI_WO] = 1;
            info[gk::RPI_NT] = 1;
            info[gk::RPI_R2E] = cp.r2e;
            info[gk::RPI_L2E] = cp.l2e;
            info[gk::RPI_LDS] = cp.lds;
            info[gk::RPI_NRES2] = cp.nres2;
            info[gk::RPI_WT] = gk::CB_WT;
            info[gk::RPI_BLK] = 1;
        }
    }
    // op_precond_sten's conditions, without its collective (the smallest slab of
    // a multi-rank context is gathered at its first solve)
    int cs = c->pkind == GK_PREC_CHEB && c->tune_cheb_sten && c->pdeg <= gk::CF_LMAX && c->N >= gk::CF_PTS &&
             c->tune_cheb_fused && c->N % 2 == 0 &&
             (i64)c->N * std::max(c->nlines, c->max_lines) * 8 < (1LL << 31);
    if (cs && collective(c) && c->nranks > 1) cs = c->min_lines == 0 ? -1 : (c->min_lines >= c->pdeg + 1 ? 1 : 0);
    info[gk::RPI_CHEB_STEN] = cs;
    return GK_OK;
}

}  // extern "C"

// ------------------------------------------------- stateless kernel API ----

namespace gkh __attribute__((visibility("hidden"))) {
// Device scratch for the stateless calls: NSLOT partial slabs + a scalar area.
double *g_scratch[64] = {nullptr};

int stateless_ctx(gk_ctx &c, int N, int nlines, i64 n, void *stream) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return set_err(GK_ERR_ARG, "device id %d", dev);
    if (g_scratch[dev] == nullptr) {
        if (hipMalloc(&g_scratch[dev], sizeof(double) * (NSLOT * gk::NPMAX + 64)) != hipSuccess)
            return set_err(GK_ERR_NOMEM, "scratch allocation failed");
    }
    c.dev = dev;
    c.N = N;
    c.nlines = nlines;
    c.nloc = n;
    c.max_lines = nlines;
    c.st = reinterpret_cast<hipStream_t>(stream);
    c.red = g_scratch[dev];
    c.scal = g_scratch[dev] + NSLOT * gk::NPMAX;
    set_geometry(&c);
    return GK_OK;
}

void release_stateless(gk_ctx &c) {
    // nothing owned: keep the destructor-free fields from being freed
    c.red = nullptr;
    c.scal = nullptr;
    c.st = nullptr;
}

bool aligned16(const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace gkh

extern "C" {

int gk_poisson5(int nside, int nlines, const double *x, const double *hlo, const double *hhi, double *y,
                void *stream) {
    if (nside < 2 || nlines < 1 || x == nullptr || y == nullptr) return set_err(GK_ERR_ARG, "bad poisson5 args");
    if (!aligned16(x) || !aligned16(y) || !aligned16(hlo) || !aligned16(hhi))
        return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_ctx c;
    CHK(stateless_ctx(c, nside, nlines, (i64)nside * nlines, stream));
    const int rc = stencil_plain_raw(&c, x, hlo, hhi, y);
    release_stateless(c);
    return rc;
}

int gk_precond_apply(int nside, int kind, const double *params, int degree, const double *r, double *z,
                     double *scratch, void *stream) {
    if (nside < 2 || r == nullptr || z == nullptr) return set_err(GK_ERR_ARG, "bad precond args");
    if (kind == GK_PREC_MG) return set_err(GK_ERR_ARG, "multigrid needs a context: gk_set_precond(ctx, GK_PREC_MG, ...)");
    if (!aligned16(r) || !aligned16(z) || !aligned16(scratch))
        return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    const i64 n = (i64)nside * nside;
    gk_ctx c;
    CHK(stateless_ctx(c, nside, nside, n, stream));
    int rc = gk_set_precond(&c, kind, params, params ? 2 : 0, degree);
    if (rc == GK_OK && scratch == nullptr && kind == GK_PREC_CHEB)
        rc = set_err(GK_ERR_ARG, "Chebyshev needs 3 scratch vectors");
    if (rc == GK_OK) {
        // op_precond expects z = A v already formed for a step; here the input
        // IS the residual, so run the preconditioner sweeps directly on r.
        c.aux = scratch;
        c.dA = scratch ? scratch + n : nullptr;
        c.dB = scratch ? scratch + 2 * n : nullptr;
        rc = op_Minv_or_copy(&c, r, z);
    }
    c.aux = c.dA = c.dB = nullptr;
    release_stateless(c);
    return rc;
}

int gk_mgs_project(long long n, double *w, const double *va, double *result, void *stream) {
    if (n < 1 || w == nullptr || va == nullptr || result == nullptr) return set_err(GK_ERR_ARG, "bad args");
    if (!aligned16(w) || !aligned16(va)) return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_ctx c;
    CHK(stateless_ctx(c, 2, 1, n, stream));
    int rc = GK_OK;
    if (hipMemsetAsync(result, 0, sizeof(double), c.st) != hipSuccess) rc = set_err(GK_ERR_HIP, "memset");
    if (rc == GK_OK) rc = proj(&c, gk::PJ_DOT, w, nullptr, va, nullptr, 0, slot(&c, 0), nullptr, 1.0);
    if (rc == GK_OK) rc = proj(&c, gk::PJ_AXPY, w, va, nullptr, slot(&c, 0), c.np_pj, nullptr, result, 1.0);
    release_stateless(c);
    return rc;
}

int gk_dot(long long n, const double *a, const double *b, double *result, void *stream) {
    if (n < 1 || a == nullptr || b == nullptr || result == nullptr) return set_err(GK_ERR_ARG, "bad args");
    if (!aligned16(a) || !aligned16(b)) return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_ctx c;
    CHK(stateless_ctx(c, 2, 1, n, stream));
    int rc = proj(&c, gk::PJ_DOT, const_cast<double *>(a), nullptr, b, nullptr, 0, slot(&c, 0), nullptr, 1.0);
    if (rc == GK_OK) rc = finalize(&c, slot(&c, 0), c.np_pj, result, 0);
    release_stateless(c);
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ Lanczos --

namespace gkh __attribute__((visibility("hidden"))) {
// Number of eigenvalues of the symmetric tridiagonal (a, b) smaller than x (Sturm count).
int sturm_count(const std::vector<double> &a, const std::vector<double> &b, double x) {
    int cnt = 0;
    double q = 1.0;
    for (size_t i = 0; i < a.size(); ++i) {
        const double bb = i ? b[i - 1] * b[i - 1] : 0.0;
        q = a[i] - x - (i ? bb / q : 0.0);
        if (q == 0.0) q = -1e-300;
        if (q < 0.0) ++cnt;
    }
    return cnt;
}

double tridiag_eig(const std::vector<double> &a, const std::vector<double> &b, int which) {
    double lo = a[0], hi = a[0];
    for (size_t i = 0; i < a.size(); ++i) {
        const double r = (i ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < a.size() ? std::fabs(b[i]) : 0.0);
        lo = std::min(lo, a[i] - r);
        hi = std::max(hi, a[i] + r);
    }
    for (int it = 0; it < 200; ++it) {  // bisection on the Sturm count
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(a, b, mid) > which) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
}

int dot_host(gk_ctx *c, const double *a, const double *b, double *out) {
    CHK(proj(c, gk::PJ_DOT, const_cast<double *>(a), nullptr, b, nullptr, 0, slot(c, 3), nullptr, 1.0));
    CHK(allreduce(c, slot(c, 3), c->np_pj));
    CHK(finalize(c, slot(c, 3), c->np_pj, c->scal + 6, 0));
    return d2h_sync(c, out, c->scal + 6, 1);
}

int axpy_host(gk_ctx *c, double *y, double a, const double *x) {
    gk::k_axpy_host<<<c->nblk_stream, gk::TPB, 0, c->st>>>(y, a, x, c->nloc);
    LAUNCHCHK();
    return GK_OK;
}
}  // namespace gkh

extern "C" int gk_lanczos_bounds(gk_ctx *c, int k, double *lmin, double *lmax) {
    CHK(check_ctx(c));
    if (k < 2 || k > 1000 || lmin == nullptr || lmax == nullptr) return set_err(GK_ERR_ARG, "bad Lanczos args");
    HIPCHK(hipSetDevice(c->dev));
    c->cycle_mgs = c->cycle_hh = false;  // uses the work vectors
    double *qprev = c->dA, *q = c->dB, *w = c->vj;
    CHK(fill_hash(c, q, 12345ull));
    HIPCHK(hipMemsetAsync(qprev, 0, sizeof(double) * c->nloc, c->st));
    double nq;
    CHK(dot_host(c, q, q, &nq));
    CHK(axpy_host(c, q, 1.0 / std::sqrt(nq) - 1.0, q));  // q /= ||q||
    std::vector<double> al, be;
    double beta = 0.0;
    for (int it = 0; it < k; ++it) {
        CHK(op_A(c, q, w, gk::ACC_NONE, nullptr, nullptr));  // w = A q
        if (beta != 0.0) CHK(axpy_host(c, w, -beta, qprev));
        double alpha;
        CHK(dot_host(c, w, q, &alpha));
        CHK(axpy_host(c, w, -alpha, q));
        double b2;
        CHK(dot_host(c, w, w, &b2));
        al.push_back(alpha);
        beta = std::sqrt(b2);
        if (beta == 0.0 || it == k - 1) break;
        be.push_back(beta);
        std::swap(qprev, q);                                // q_{j-1} <- q_j
        HIPCHK(hipMemcpyAsync(q, w, sizeof(double) * c->nloc, hipMemcpyDeviceToDevice, c->st));
        CHK(axpy_host(c, q, 1.0 / beta - 1.0, q));          // q_{j+1} = w / beta
    }
    be.resize(al.size() > 0 ? al.size() - 1 : 0);
    *lmin = tridiag_eig(al, be, 0);
    *lmax = tridiag_eig(al, be, (int)al.size() - 1);
    CHK(sync_st(c));
    return GK_OK;
}

// ------------------------------------------- device vector primitives -------
// Short-recurrence solvers (pcg_omp src/cg.f90:154-234, pbicgstab_omp
// src/bicgstab.f90:91-182) on context-resident vectors: id 0 = x, 1 = b,
// 2 .. m+2 = scratch (the Krylov columns).

namespace gkh __attribute__((visibility("hidden"))) {
double *vec_of(gk_ctx *c, int id) {
    if (id == GK_VEC_X) return c->x;
    if (id == GK_VEC_B) return c->b;
    if (id >= 2 && id <= c->m + 2) return c->V + (i64)(id - 2) * c->ld;
    return nullptr;
}
}  // namespace gkh

extern "C" {

int gk_vec_count(gk_ctx *c, int *count) {
    CHK(check_ctx(c));
    *count = c->m + 3;
    return GK_OK;
}

int gk_vec_apply(gk_ctx *c, int what, int in, int out) {
    CHK(check_ctx(c));
    double *vi = vec_of(c, in), *vo = vec_of(c, out);
    if (vi == nullptr || vo == nullptr || in == out || what < 0 || what > 2)
        return set_err(GK_ERR_ARG, "bad gk_vec_apply(%d, %d, %d)", what, in, out);
    HIPCHK(hipSetDevice(c->dev));
    c->cycle_mgs = c->cycle_hh = false;
    if (what == 2 && c->pkind != GK_PREC_IDENTITY)  // out = A M^-1 in, the right-preconditioned step's operator
        return op_right(c, vi, vo, gk::ACC_NONE, nullptr, nullptr);
    if (what != 1)  // A in (what = 2 with the identity preconditioner is A itself)
        return op_A(c, vi, vo, gk::ACC_NONE, nullptr, nullptr);
    const double *src = vi;
    if (c->pkind != GK_PREC_IDENTITY) {  // the sweeps read their input from z
        HIPCHK(hipMemcpyAsync(c->z, vi, sizeof(double) * c->nloc, hipMemcpyDeviceToDevice, c->st));
        src = c->z;
    }
    return op_Minv_or_copy(c, src, vo);
}

int gk_vec_dot(gk_ctx *c, int a, int b, double *result) {
    CHK(check_ctx(c));
    double *va = vec_of(c, a), *vb = vec_of(c, b);
    if (va == nullptr || vb == nullptr || result == nullptr) return set_err(GK_ERR_ARG, "bad gk_vec_dot");
    HIPCHK(hipSetDevice(c->dev));
    return dot_host(c, va, vb, result);
}

int gk_vec_lincomb(gk_ctx *c, int form, int out, int a, int b, int cc, double s1, double s2) {
    CHK(check_ctx(c));
    double *vo = vec_of(c, out);
    const double *va = vec_of(c, a), *vb = vec_of(c, b), *vc = vec_of(c, cc);
    const bool need_a = form != GK_LC_ZERO, need_b = form == GK_LC_AXPY || form == GK_LC_AXPY2 ||
                                                    form == GK_LC_XPAYMZ;
    const bool need_c = form == GK_LC_AXPY2 || form == GK_LC_XPAYMZ;
    if (vo == nullptr || form < 0 || form > GK_LC_ZERO || (need_a && va == nullptr) || (need_b && vb == nullptr) ||
        (need_c && vc == nullptr))
        return set_err(GK_ERR_ARG, "bad gk_vec_lincomb");
    HIPCHK(hipSetDevice(c->dev));
    gk::k_lincomb<<<c->nblk_stream, gk::TPB, 0, c->st>>>(form, vo, va, vb, vc, s1, s2, c->nloc);
    LAUNCHCHK();
    return GK_OK;
}

}  // extern "C"
