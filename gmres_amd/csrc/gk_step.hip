// gk_step.hip -- what every Arnoldi path launches, and the MGS-R cycle: the streaming
// launches (projection, scale, x update, Gram; kernels in gk_step_kernels.hpp, which this
// unit alone includes), the resident step's planning and launch for a context, the
// launch-path chains and their graphs, and the C-ABI entries gk_mgs_* / gk_update_x.  The
// Householder cycle (gk_hh.hip) runs on the same launches.  Declarations: gk_host.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gk_blk.hpp"
#include "gk_cb.hpp"
#include "gk_cgs.hpp"
#include "gk_host.hpp"
#include "gk_resident.hpp"
#include "gk_step_kernels.hpp"

using namespace gkh;
using gk::ResPlan;

namespace gkh __attribute__((visibility("hidden"))) {

// -------------------------------------------------------------- launches ---
// T: the type va / vb are stored in (float: the FP32 basis, PJ_AXPY_DOT / PJ_AXPY_NORM only)
template <bool NT, int U, class T>
void launch_proj_u(gk_grid *c, int mode, double *w, const T *va, const T *vb, const double *pin, int npin,
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
void launch_proj(gk_grid *c, int mode, double *w, const T *va, const T *vb, const double *pin, int npin,
                 double *pout, double *hslot, double coef, i64 tail0, int hstore) {
    // loads in flight per thread and array: one trip per thread when the vector is small, else 2
    const i64 per_thread = (c->nloc / 2 + (i64)c->np_pj * gk::TPB - 1) / ((i64)c->np_pj * gk::TPB);
    if (per_thread > 4)
        launch_proj_u<NT, 2>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    else
        launch_proj_u<NT, 4>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
}

// (T is named, never deduced: callers pass nullptr for the column a mode does not read)
template <class T>
int proj_t(gk_grid *c, int mode, double *w, const std::common_type_t<T> *va, const std::common_type_t<T> *vb,
           const double *pin, int npin, double *pout, double *hslot, double coef, i64 tail0 = 0, int hstore = 0) {
    if (!std::is_same<T, double>::value && mode != gk::PJ_AXPY_DOT && mode != gk::PJ_AXPY_NORM)
        return set_err(GK_ERR_STATE, "projection mode %d on float columns", mode);
    ProfScope ps(c, GK_KID_PROJ);
    if (nt_cols(c))
        launch_proj<true>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    else
        launch_proj<false>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
    LAUNCHCHK();
    return GK_OK;
}

int proj(gk_grid *c, int mode, double *w, const double *va, const double *vb, const double *pin, int npin,
         double *pout, double *hslot, double coef, i64 tail0, int hstore) {
    return proj_t<double>(c, mode, w, va, vb, pin, npin, pout, hslot, coef, tail0, hstore);
}

int scale(gk_ctx *c, double *out, const double *w, const double *pin, int npin, double *hslot, double *hcopy,
          const double *hsrc, int ncopy, bool pin_norm) {
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

int fill_hash(gk_ctx *c, double *x, unsigned long long seed) {
    gk::k_fill_hash<<<c->nblk_stream, gk::TPB, 0, c->st>>>(x, c->nloc, c->g0, seed);
    LAUNCHCHK();
    return GK_OK;
}

int finalize(gk_grid *c, const double *pin, int npin, double *out, int take_sqrt) {
    ProfScope ps(c, GK_KID_OTHER);
    gk::k_finalize<<<1, gk::TPB, 0, c->st>>>(pin, npin, out, take_sqrt);
    LAUNCHCHK();
    return GK_OK;
}

// Can step j run as one resident launch, and with which variant?  Needs an
// in-launch reduction path: single rank, or the device exchange (RCCL and the
// host-side local group cannot be driven from inside a kernel).
bool res_plan(gk_ctx *c, ResPlan &p, bool hh) {
    if (c->tune_res == 0 || c->res_broken || c->m > gk::RHMAX || c->res_cus <= 0 || c->res_gath == nullptr)
        return false;
    if (collective(c) && !(c->xs_on && c->nranks > 1)) return false;
    // Several resident launches on one device spin on each other's partials, so
    // their streams must run concurrently -- HIP promises nothing about how
    // streams map to hardware queues.  Auto mode assumes one context per device.
    if (c->tune_res < 0 && c->res_share > 1) return false;
    const int gmax = std::max(1, std::min(gk::RGMAX, c->res_cus / std::max(1, c->res_share)));
    const int cap = c->tune_res_r2 > 0 ? c->tune_res_r2 : gk::RES_R2_BIG;
    gk::plan_resident(c->nloc, gmax, cap, c->tune_res_wonly, hh, nt_cols(c), p, c->tune_res_pc, c->tune_res_blk,
                      c->tune_res_pf, c->tune_res_pipe, c->tune_res_carry);
    if (c->nranks > 1) p.carry = 0;  // the carried pass is the single-rank launches' (gk_resident.hip)
    if (p.wo && !hh && c->m + 1 > gk::WO_HMAX) return false;  // its H column: WO_HMAX entries of LDS
    return true;
}

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

// One resident launch (gk::ResArgs::mode):
//  RES_MGS: the MGS cascade of step j + norm + scale; pin/npin = the
//    (all-reduced) partial slab of the first dot <w, V(:,1)>; H column to hs/hcopy.
//  RES_HH_UP: w = P_j..P_1 w (pin = <w, P_1>); hs[0] = ||w(j+1:n)||^2.
//  RES_HH_DOWN: w = P_1..P_j w (no pin).
//  flags (w-only variant, p.wo): RESF_CLOSE_HH -- RES_HH_UP also makes P(:,j+1) and
//    writes w(1:j+1) to c->hb (one more exchange); RESF_UNIT_INIT -- RES_HH_DOWN builds
//    its unit input e_{unit_g} itself.  RESF_PIN_LOCAL (any variant, N ranks on the device
//    exchange): pin holds this rank's partials, the launch sums them across ranks.
int res_step(gk_ctx *c, int j, const ResPlan &p, const double *pin, int npin, double *hs, double *hcopy, int mode,
             double *w, i64 unit_g, int flags) {
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
    CHK(sync_harvest(c));
    std::memcpy(host, c->hcol_host, sizeof(double) * count);
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
    CHK(sync_harvest(c));
    G.assign((size_t)ncols * ncols, 0.0);
    for (int p = 0; p < np; ++p) {
        G[(size_t)pr[p].y * ncols + pr[p].x] = flat[p];
        G[(size_t)pr[p].x * ncols + pr[p].y] = flat[p];
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
    const HCol h = hcol_of(c, j);
    int s0 = 0, s1 = 1;
    const int np_total = 2 * j;
    for (int p = 0; p < np_total; ++p) {
        const int i = p % j;
        CHK(allreduce(c, slot(c, s0), np));
        const T *va = vcol<T>(c, i);
        const int first_pass = p < j;
        if (p + 1 < np_total) {
            const T *vb = vcol<T>(c, (p + 1) % j);
            CHK(proj_t<T>(c, gk::PJ_AXPY_DOT, c->w, va, vb, slot(c, s0), np, slot(c, s1), h.dev + i, 1.0, 0,
                          first_pass));
        } else {
            CHK(proj_t<T>(c, gk::PJ_AXPY_NORM, c->w, va, nullptr, slot(c, s0), np, slot(c, s1), h.dev + i, 1.0, 0,
                          first_pass));
        }
        np = c->np_pj;
        std::swap(s0, s1);
    }
    CHK(allreduce(c, slot(c, s0), np));
    return scale_col(c, j, slot(c, s0), np, h.dev + j, h.map, h.dev, j);
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
    const int G = c->np_pj;
    const HCol h = hcol_of(c, j);
    const bool nt = nt_cols(c);
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
            HIPCHK(gk::cgs_axpy(sweep == 1, nt, G, c->w, c->V, c->ld, j, c->nloc, c->cgs_s, h.dev, sweep == 0,
                                slot(c, 0), c->st));
        }
    }
    CHK(allreduce(c, slot(c, 0), G));
    return scale_col(c, j, slot(c, 0), G, h.dev + j, h.map, h.dev, j);
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

// The head of gk_update_x / gk_hh_update_x: the checks, the device, y(1:n_out) to ydev.  Their
// tail is sync_harvest.
int update_begin(gk_ctx *c, const double *y, int n_out) {
    CHK(check_ctx(c));
    CHK(check_nout(c, n_out));
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipMemcpyAsync(c->ydev, y, sizeof(double) * n_out, hipMemcpyHostToDevice, c->st));
    return GK_OK;
}

}  // namespace gkh

// ------------------------------------------------------------------ MGS-R --

extern "C" {

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
    CHK(check_step(c, j));
    if (!c->cycle_mgs) return set_err(GK_ERR_STATE, "gk_mgs_step before gk_mgs_cycle_start");
    HIPCHK(hipSetDevice(c->dev));
    const HCol h = hcol_of(c, j);  // H(1:j+1, j) of this step
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
    const double *vj = cb ? cb_vjw(c) : vcol<double>(c, j - 1), *v1 = cb ? cb_v1w(c) : c->V;
    // w = M^-1 A V(:,j) (side right: A M^-1 V(:,j)), fused with the first dot <w, V(:,1)>
    if (right_prec(c))
        CHK(op_right(c, vj, c->w, acc, v1, slot(c, s0)));
    else
        CHK(op_precond(c, vj, c->w, false, acc, v1, slot(c, s0)));
    const int np = c->last_np;
    if (res) {  // the whole cascade + norm + scale as one resident launch
        // N ranks on the device exchange: the first dot's rank totals inside the launch
        // (GK_TUNE_RES_FOLD) instead of a k_xchg launch before it
        const bool fold = c->tune_res_fold && c->xs_on && c->nranks > 1;
        if (!fold) CHK(allreduce(c, slot(c, s0), np));
        if (cb)  // ... on float columns (k_mgs_wcb; one rank)
            CHK(cb_step(c, j, cp, slot(c, s0), np, h.dev, h.map));
        else
            CHK(res_step(c, j, rp, slot(c, s0), np, h.dev, h.map, gk::RES_MGS, nullptr, -1,
                         fold ? RESF_PIN_LOCAL : 0));
    } else {
        // Launch path: RCCL ranks (or one rank with the resident step off) replay the
        // step's projection chain as a hipGraph captured at its first use (GK_TUNE_GRAPH).
        bool replayed = false;
        if (c->tune_graph && (c->lg == nullptr || c->xs_on)) {
            if (c->gkey != np) {
                graph_reset(c);
                c->gkey = np;
            }
            if ((int)c->gstep.size() < c->m + 1) c->gstep.resize(c->m + 1, nullptr);
            if (c->gstep[j] == nullptr) CHK(capture_step(c, j, np));
            if (c->gstep[j] != nullptr) {
                ProfScope ps(c, GK_KID_GRAPH);
                if (c->xs_on && c->gxs[j] > 0) {  // the replay's exchanges continue this context's numbering
                    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->xs_seqdev), (int)c->xs_seq, 1, c->st));
                    c->xs_seq += c->gxs[j];
                }
                HIPCHK(hipGraphLaunch(c->gstep[j], c->st));
                replayed = true;
            }
        }
        if (!replayed) CHK(mgs_chain(c, j, np));
    }
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
    CHK(check_step(c, j));
    CHK(wait_step_event(c, c->ev_step[j]));
    CHK(res_check(c));
    CHK(xs_check(c));
    const volatile double *src = hcol_of(c, j).host;
    for (int k = 0; k <= j; ++k) hcol[k] = src[k];
    return GK_OK;
}

int gk_mgs_step(gk_ctx *c, int j, double *hcol) {
    CHK(gk_mgs_step_async(c, j));
    return gk_mgs_step_wait(c, j, hcol);
}

int gk_update_x(gk_ctx *c, const double *y, int n_out) {
    CHK(update_begin(c, y, n_out));
    if (right_prec(c)) {  // x += M^-1 (V y): t = V y in w, M^-1 t in z
        CHK(update_x<false>(c, c->w, n_out));
        CHK(add_precond_sweeps(c, c->w));
    } else {
        CHK(update_x<true>(c, c->x, n_out));
    }
    return sync_harvest(c);
}

int gk_mgs_verr(gk_ctx *c, int n_out, int zero_last, double *v_err) {
    CHK(check_ctx(c));
    CHK(check_nout(c, n_out));
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

}  // extern "C"
