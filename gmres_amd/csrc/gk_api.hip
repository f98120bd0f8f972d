// gk_api.hip -- C-ABI implementation of include/gmres_hip.h (libgmres_hip.so): the
// context's lifetime, setters and accessors, tuning, profiling, the plan and info queries,
// the stateless API, Lanczos and the gk_vec_* primitives.  The Arnoldi launches and the
// MGS-R cycle live in gk_step.hip, the Householder cycle in gk_hh.hip, the operator and
// the preconditioner in gk_op.hip, the collectives in gk_comm.hip, the resident step's
// kernels, planner and launchers in gk_resident.hip (the blocked step in gk_blk.hip), the
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

#include "gk_cb.hpp"
#include "gk_cgs.hpp"
#include "gk_cheb.hpp"
#include "gk_host.hpp"
#include "gk_kernels.hpp"
#include "gk_mg.hpp"
#include "gk_resident.hpp"

using namespace gkh;

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
void set_geometry(gk_grid *c) {
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
    c->nt_auto = gk::nt_auto_for((i64)ml * N);
    if (npj < 1) npj = 1;
    c->np_pj = (int)npj;
    // elementwise kernels: also from the largest slab (their partial slabs are all-reduced)
    i64 nb = (nmax2 + gk::TPB - 1) / gk::TPB;
    c->nblk_stream = (int)std::min<i64>(std::max<i64>(nb, 1), 2048);
}

int check_ctx(gk_ctx *c) {
    if (c == nullptr) return set_err(GK_ERR_ARG, "null context");
    if (c->broken)
        return set_err(GK_ERR_STATE, "context broken by an earlier watchdog timeout (work never completed on its "
                                     "stream): destroy it");
    if (c->nranks > 1 && !c->comm_ok) return set_err(GK_ERR_STATE, "communicator not initialised");
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
    c->ctx = c;
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

// What gk_set_precond and gk_precond_apply refuse of (kind, params, degree) alone
static int check_precond_args(int kind, const double *params, int nparams, int degree) {
    if (kind < GK_PREC_IDENTITY || kind > GK_PREC_MG) return set_err(GK_ERR_ARG, "bad precond kind %d", kind);
    if (kind != GK_PREC_IDENTITY && (params == nullptr || nparams < 2))
        return set_err(GK_ERR_ARG, "precond needs params(1:2)");
    if (kind == GK_PREC_CHEB && (degree < 1 || degree > 64)) return set_err(GK_ERR_ARG, "bad degree %d", degree);
    if (kind == GK_PREC_CHEB && std::fabs(params[1] - params[0]) == 0.0)
        return set_err(GK_ERR_ARG, "Chebyshev interval is empty");
    return GK_OK;
}

int gk_set_precond(gk_ctx *c, int kind, const double *params, int nparams, int degree) {
    CHK(check_ctx(c));
    sr_invalidate(c);
    CHK(check_precond_args(kind, params, nparams, degree));
    if (kind == GK_PREC_MG) {  // everything checked, and the hierarchy built, before the context changes
        int sides[gk::MG_LMAX];
        if (gk::mg_levels(c->N, sides) < 2)
            return set_err(GK_ERR_ARG, "multigrid needs an even N with N / 2 >= %d (N = %d)", gk::MG_NMIN, c->N);
        if (degree < 1 || degree > gk::MG_DEG_MAX)
            return set_err(GK_ERR_ARG, "multigrid smoother degree %d outside 1..%d", degree, gk::MG_DEG_MAX);
        if (std::fabs(params[1] - params[0]) == 0.0) return set_err(GK_ERR_ARG, "multigrid smoother interval is empty");
        if (c->nranks > 1 || c->comm != nullptr || c->lg != nullptr || c->xs_on || c->line0 != 0 || c->nlines != c->N)
            return set_err(GK_ERR_STATE, "multigrid needs the whole grid on one rank (no communicator)");
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

// A := A_poisson + sigma I.  The open cycle's basis and a running gk_sr_* solve belong to the
// other operator; captured steps hold diag (and the multigrid levels' coefficients) by value.
int gk_set_shift(gk_ctx *c, double sigma) {
    CHK(check_ctx(c));
    if (!(sigma >= 0.0) || !(sigma <= 1e12))  // NaN fails both
        return set_err(GK_ERR_ARG, "shift %g outside 0 .. 1e12", sigma);
    sr_invalidate(c);
    c->cycle_mgs = c->cycle_hh = false;
    if (sigma != c->shift) graph_reset(c);
    c->shift = sigma;
    mg_refresh(c);
    return GK_OK;
}

int gk_get_shift(gk_ctx *c, double *sigma) {
    CHK(check_ctx(c));
    if (sigma == nullptr) return set_err(GK_ERR_ARG, "null sigma");
    *sigma = c->shift;
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
    return sync_harvest(c);
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
    return sync_harvest(c);
}

int gk_res_plan_query(long long nloc, int cus, int share, int hh, int nt, int block, long long *info) {
    if (info == nullptr || nloc < 2 || cus < 1 || share < 1 || (block != 1 && block != 2 && block != 4))
        return set_err(GK_ERR_ARG, "bad plan query");
    const int gmax = std::max(1, std::min(gk::RGMAX, cus / share));
    gk::ResPlan p;
    gk::plan_resident(nloc, gmax, gk::RES_R2_BIG, -1, hh != 0, nt < 0 ? gk::nt_auto_for(nloc) : nt != 0, p, -1, block);
    gk::plan_info(p, true, info);
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
    mg_info_fill(sides, nl, gk::mg_coarse_degree(sides[nl - 1], 0.0, &lo, &hi), 0, info);
    return GK_OK;
}

int gk_mg_info(gk_ctx *c, int *info) {
    CHK(check_ctx(c));
    if (info == nullptr) return set_err(GK_ERR_ARG, "null info");
    if (c->pkind != GK_PREC_MG || c->mg.size() < 2) return set_err(GK_ERR_STATE, "no multigrid preconditioner set");
    int sides[gk::MG_LMAX];
    const int nl = (int)c->mg.size();
    for (int l = 0; l < nl; ++l) sides[l] = c->mg[l].g.N;
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
    gk::ResPlan p;
    const bool on = !(hh == 0 && cgs_on(c)) && res_plan(c, p, hh != 0);  // a CGS2 context's MGS step: launch by launch
    gk::plan_info(p, on, info);
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

// The bare grid of a stateless call: nothing owned, the caller's stream
int stateless_grid(gk_grid &c, int N, int nlines, i64 n, void *stream) {
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

bool aligned16(const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace gkh

extern "C" {

int gk_poisson5_shift(int nside, int nlines, double sigma, const double *x, const double *hlo, const double *hhi,
                      double *y, void *stream) {
    if (nside < 2 || nlines < 1 || x == nullptr || y == nullptr) return set_err(GK_ERR_ARG, "bad poisson5 args");
    if (!(sigma >= 0.0) || !(sigma <= 1e12)) return set_err(GK_ERR_ARG, "shift %g outside 0 .. 1e12", sigma);
    if (!aligned16(x) || !aligned16(y) || !aligned16(hlo) || !aligned16(hhi))
        return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_grid c;
    CHK(stateless_grid(c, nside, nlines, (i64)nside * nlines, stream));
    c.shift = sigma;
    return stencil_plain_raw(&c, x, hlo, hhi, y);
}

int gk_poisson5(int nside, int nlines, const double *x, const double *hlo, const double *hhi, double *y,
                void *stream) {
    return gk_poisson5_shift(nside, nlines, 0.0, x, hlo, hhi, y, stream);
}

int gk_precond_apply(int nside, int kind, const double *params, int degree, const double *r, double *z,
                     double *scratch, void *stream) {
    if (nside < 2 || r == nullptr || z == nullptr) return set_err(GK_ERR_ARG, "bad precond args");
    if (kind == GK_PREC_MG) return set_err(GK_ERR_ARG, "multigrid needs a context: gk_set_precond(ctx, GK_PREC_MG, ...)");
    if (!aligned16(r) || !aligned16(z) || !aligned16(scratch))
        return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    const i64 n = (i64)nside * nside;
    gk_grid c;
    CHK(stateless_grid(c, nside, nside, n, stream));
    CHK(check_precond_args(kind, params, params ? 2 : 0, degree));
    if (scratch == nullptr && kind == GK_PREC_CHEB) return set_err(GK_ERR_ARG, "Chebyshev needs 3 scratch vectors");
    c.pkind = kind;
    if (params != nullptr) {
        c.p0 = params[0];
        c.p1 = params[1];
    }
    c.pdeg = degree;
    // op_precond expects z = A v already formed for a step; here the input
    // IS the residual, so run the preconditioner sweeps directly on r.
    c.aux = scratch;
    c.dA = scratch ? scratch + n : nullptr;
    c.dB = scratch ? scratch + 2 * n : nullptr;
    return grid_Minv_or_copy(&c, r, z);
}

int gk_mgs_project(long long n, double *w, const double *va, double *result, void *stream) {
    if (n < 1 || w == nullptr || va == nullptr || result == nullptr) return set_err(GK_ERR_ARG, "bad args");
    if (!aligned16(w) || !aligned16(va)) return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_grid c;
    CHK(stateless_grid(c, 2, 1, n, stream));
    if (hipMemsetAsync(result, 0, sizeof(double), c.st) != hipSuccess) return set_err(GK_ERR_HIP, "memset");
    CHK(proj(&c, gk::PJ_DOT, w, nullptr, va, nullptr, 0, slot(&c, 0), nullptr, 1.0));
    return proj(&c, gk::PJ_AXPY, w, va, nullptr, slot(&c, 0), c.np_pj, nullptr, result, 1.0);
}

int gk_dot(long long n, const double *a, const double *b, double *result, void *stream) {
    if (n < 1 || a == nullptr || b == nullptr || result == nullptr) return set_err(GK_ERR_ARG, "bad args");
    if (!aligned16(a) || !aligned16(b)) return set_err(GK_ERR_ARG, "device pointers must be 16-byte aligned");
    gk_grid c;
    CHK(stateless_grid(c, 2, 1, n, stream));
    CHK(proj(&c, gk::PJ_DOT, const_cast<double *>(a), nullptr, b, nullptr, 0, slot(&c, 0), nullptr, 1.0));
    return finalize(&c, slot(&c, 0), c.np_pj, result, 0);
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
