// gk_host.hpp -- internal header of the host-side units of libgmres_hip.so
// (gk_api.hip, gk_step.hip, gk_hh.hip, gk_op.hip, gk_comm.hip, gk_sr_api.hip); never installed.
// The context, the error / check macros, the profiling scope and the helpers that cross units.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gmres_hip.h"
#include "gk_res.hpp"

using gk::i64;

namespace gk {
struct SrDev;
struct SrMirror;
struct ResPlan;  // gk_resident.hpp
struct CbPlan;   // gk_cb.hpp
}  // namespace gk

// In-process communicator: several contexts of one process (e.g. ranks
// sharing one GPU in tests) driven by one host thread each.  Collectives are
// a host barrier + HIP event ordering + device copies/sums; the message
// pattern is exactly the RCCL one (same counts, same roots, same halos).
struct gk_group {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    bool broken = false;
    std::vector<gk_ctx *> members;
    std::vector<const double *> ptrs;
};

// One slab of grid lines and all that the operator, the preconditioner sweeps and the
// streaming launches read of it: everything that takes a gk_grid * (set_geometry, stencil,
// grid_sweeps, cheb_fused, proj, finalize, ...) runs on these members alone.  A bare grid --
// a multigrid level, a stateless call's stack object -- owns nothing and has ctx null: no
// neighbour (halo and collective do nothing, the boundary halos are null) and no profiling
// events.  A context (gk_ctx) is a grid whose ctx points at itself.
struct gk_grid {
    gk_ctx *ctx = nullptr;  // the context this grid is the base of: its communicators and profiling events
    int dev = 0, N = 0, line0 = 0, nlines = 0;
    int max_lines = 0;  // largest slab of any rank (0: nlines)
    i64 nloc = 0, ld = 0, g0 = 0;
    hipStream_t st = nullptr;
    // launch geometry (set_geometry) and the tunings it reads
    int vec = 2, JT = 16;
    dim3 sgrid;
    int sr_JT = 64;  // the short-recurrence marches' geometry (gk_sr_*)
    dim3 sr_sgrid;
    int np_sr = 0;
    int np_st = 0, np_pj = 0, nblk_stream = 0;
    bool nt_auto = false;
    int tune_nt = -1, tune_pj_blocks = 0, tune_st_blocks = 0, tune_sr_blocks = 0;  // tune_nt: -1 auto
    int last_np = 0;  // partial count written by the last ACC-carrying sweep
    int res_cus = 0;  // compute units of the device
    // operator and preconditioner
    double shift = 0.0;  // the operator is A_poisson + shift I (gk_set_shift; a multigrid level's: 4^l times it)
    int pkind = GK_PREC_IDENTITY, pdeg = 8;
    double p0 = 8.2, p1 = 0.2;
    int tune_cheb_fused = 1;  // temporal-blocked Chebyshev sweeps (single slab)
    int tune_cheb_sten = 1;   // the Arnoldi step's pass forms z = A v itself (stage 0)
    double *aux = nullptr, *dA = nullptr, *dB = nullptr;  // the Chebyshev sweeps' work vectors
    double *red = nullptr;   // NSLOT * NPMAX partial slabs
    double *scal = nullptr;  // 8 scalars
};

// One level of the GK_PREC_MG hierarchy (gk_op.hip: mg_build / mg_apply / mg_free).  g is a
// bare grid -- the level's side, the parent's device and stream, set_geometry and the level's
// Chebyshev smoother -- that the stencil and the sweeps run on; the vectors are carved from
// the parent's mg_buf (level 0 smooths on the parent's aux, dA, dB).
struct gk_mg_level {
    gk_grid g;
    double *r = nullptr, *e = nullptr;                // level > 0: its input (restricted residual) and result
    double *z = nullptr, *t = nullptr, *d = nullptr;  // level < L: iterate, residual, post-smoothing correction
};

struct gk_ctx : gk_grid {
    int m = 0;
    // HBM residents
    double *V = nullptr;  // (m+1) columns, stride ld
    double *w = nullptr, *z = nullptr;
    double *x = nullptr, *b = nullptr, *vj = nullptr, *hlo = nullptr, *hhi = nullptr;
    double *dh = nullptr;  // deep halos of the Chebyshev pass inputs: [3 vectors][lo, hi][CF_HMAX lines][N]
    double *zline = nullptr;  // N zeros (the short-recurrence marches' line past a physical boundary)
    double *hcol = nullptr;  // m+2 Hessenberg column / scalars
    double *ydev = nullptr;  // m+1
    double *hb = nullptr;    // m+2 Householder broadcast buffer
    double *hcol_host = nullptr;  // pinned
    double *hall = nullptr;       // device: per-step Hessenberg columns, m slots of m+2
    double *hallh = nullptr;      // mapped pinned host mirror of hall (written by k_scale)
    double *hallh_dev = nullptr;  // its device address
    std::vector<hipEvent_t> ev_step;  // completion of step j
    double *Vb = nullptr;    // Householder verr basis (lazy)
    double *gram_slab = nullptr, *gram_out = nullptr;
    short2 *gram_pairs = nullptr;
    int gram_nblk = 0;
    // preconditioner
    int side = GK_SIDE_LEFT;   // MGS-R: left (the reference) or right preconditioning (gk_set_precond_side)
    int tune_right_fused = 1;  // side right, cbpr2, one rank: w = A M^-1 v as one march (k_right_cbpr2)
    int basis = GK_BASIS_F64;  // MGS-R: storage precision of the Krylov columns (gk_set_basis_precision, gk_cb.hpp)
    int orth = GK_ORTH_MGSR;   // MGS-R cycle: the step's orthogonalisation (gk_set_orthogonalization, gk_cgs.hpp)
    int cgs_kb = 8;            // CGS2: columns a dots workgroup batches (gk_create: GK_CGS_KB in the environment)
    double *cgs_slab = nullptr, *cgs_s = nullptr;  // CGS2 (lazy): the dots' partials [m][np_pj], s[m]
    i64 cgs_cap = 0;                               // doubles cgs_slab holds
    std::vector<gk_mg_level> mg;                   // GK_PREC_MG: levels 0 .. L (empty otherwise)
    double *mg_buf = nullptr;                      // ... their vectors, one allocation
    int mg_cdeg = 0;                               // ... the coarsest level's sweep count
    double mg_p0 = 0.0, mg_p1 = 0.0;               // ... level 0's smoother interval as gk_set_precond gave it
    int mg_deg = 0;                                // ... and the smoother degree (mg_refresh)
    int tune_mg_fused = 1;                         // GK_TUNE_MG_FUSED: residual and restriction in one march
    // decomposition / comm
    int nranks = 1, rank = 0;
    int min_lines = 0;  // smallest slab of any rank (0: not gathered yet; ensure_min_lines)
    ncclComm_t comm = nullptr;
    bool comm_ok = false;
    gk_group *lg = nullptr;  // in-process group (GK local comm), else RCCL
    hipEvent_t lev_a = nullptr, lev_b = nullptr;
    double *lscratch = nullptr;
    // device exchange (xgmi back-end, gk_comm_init_xgmi / gk_xchg_*)
    gk::u64 *xs_buf = nullptr;  // own receive region, uncached HBM
    i64 xs_words = 0;
    gk::XsPeers xs_peers{};     // every rank's region, mapped here
    std::vector<void *> xs_mapped;
    bool xs_ready = false, xs_on = false, xs_broken = false;
    unsigned xs_seq = 0, xs_hseq = 0;
    int *xs_err = nullptr, *xs_err_dev = nullptr;  // mapped pinned flag
    long long xs_tick_per_ms = 100000;
    int xs_timeout_ms = 20000;
    gk::u64 xs_timeout = 0;
    // resident MGS-R step (gk::k_mgs_res): one persistent launch per Arnoldi step
    gk::u64 *res_gath = nullptr;                    // [RES_KMAX values][2][RGMAX][2] all-gather granules
    double *res_gm = nullptr;                       // blocked step: the cycle's Gram table [m+1][RES_SMAX]
    int tune_res_blk = 1;                           // blocked-projection MGS step: S (1 = strict MGS-R)
    int tune_res_pf = 0;                            // strict MGS step on the blocked kernel's LDS prefetch (S = 1)
    int pend_res_blk = 0, pend_res_pf = -1;         // requested mid-cycle: applied at the next cycle start
    int watchdog_ms = 0;                            // host watchdog of stream waits (0: from the device deadlines)
    bool broken = false;                            // the watchdog fired: a kernel of this context never completed
    unsigned *hold_word = nullptr, *hold_word_dev = nullptr;  // gk_debug_hold_stream's mapped word
    int *res_err = nullptr, *res_err_dev = nullptr;  // mapped deadline flag
    unsigned res_tag = 1;                           // next granule tag (never 0)
    int tune_res = -1;                              // -1 auto, 0 off, 1 on where possible
    int tune_res_r2 = 0;                            // cap of resident double2 per thread (0 = auto)
    int tune_res_pipe = -1;                         // w-only MGS step: pipelined pass (-1: the build's default)
    int tune_res_carry = -1;                        // ... its ring's head carried across the all-gather (-1: the build's)
    int tune_res_wonly = -1;                        // large slabs: w-only variant (-1: by the byte model)
    int tune_verr_order = 1;                        // v_err diagnostics in the reference's dot order
    int tune_hh_fuse = 1;                           // Householder step: small launches folded into the chains
    int tune_hh_norm_order = 0;                     // Householder: the reflector norms in flang-rt's order (1 rank)
    int res_share = 1;                              // contexts sharing this device's CUs
    int res_timeout_ms = 20000;
    bool res_broken = false;                        // a deadline was missed: launch path from then on
    gk::u64 *res_stamps = nullptr;                  // gk_profile_res_split: [RGMAX][4] ticks per workgroup
    bool res_split = false;
    gk::u64 *res_trace = nullptr;                   // gk_profile_res_trace: [RGMAX][RES_TRACE_X][2] ticks
    int res_trace_j = 0, res_trace_mode = -1;       // the traced launch: step j, mode (-1 = off)
    int res_trace_g = 0, res_trace_np = 0;          // its workgroups and exchanges
    // tuning knobs (gk_set_tuning)
    int tune_sr_two = 1;      // GK_TUNE_SR_TWO_LEVEL
    bool sr_two = false;      // this solve runs the two-level marches (set by gk_sr_start)
    int tune_spin_wait = 1;   // the per-step host wait spins on its event (0: hipEventSynchronize)
    int tune_graph = 1;       // launch-path MGS-R steps captured as hipGraphs (RCCL / no collective)
    int tune_res_qdef = -1;   // k_mgs_res NT: V_q of the LDS / streamed parts with the default policy (-1 auto)
    int tune_res_pc = -1;     // column-cache variant k_mgs_wpc: -1 by the byte model, 0 never, 1 where it fits
    int tune_res_fold = 1;    // N ranks, device exchange: the first dot's rank hop inside the MGS step launch
    std::vector<hipGraphExec_t> gstep;  // captured step j (launch path), valid for partial-slab count gkey
    std::vector<unsigned> gxs;          // device exchanges in captured step j (their sequence numbers)
    int gkey = -1;
    unsigned graph_seq0 = 0;            // xs_seq when the capture in progress began
    unsigned *xs_seqdev = nullptr;      // device: the sequence base of a replayed graph's exchanges
    bool capturing = false;   // a step is being captured: no profiling events inside it
    int prof_every = 1;       // record events in steps with j % prof_every == 0
    bool prof_on_step = true;
    // state
    bool cycle_mgs = false, cycle_hh = false;
    int hh_prec = 0;          // GK_HH_PREC_* the Householder cycle opened last was started with
    double beta0 = -1.0;
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev0, ev1;
    std::vector<int> evk;
    int nev = 0;
    double prof_ms[GK_NKID] = {0};
    long long prof_n[GK_NKID] = {0};
    // fused short-recurrence solve (gk_sr_*)
    gk::SrDev *sr_dev = nullptr;
    gk::SrMirror *sr_mir = nullptr, *sr_mir_dev = nullptr;  // mapped pinned
    double *sr_hist = nullptr;
    int sr_hist_len = 0;
    int sr_solver = -1, sr_par = 0, sr_queued = 0, sr_maxit = 0;
    std::deque<hipEvent_t> sr_pend;   // end of each queued chunk, oldest first
    std::vector<hipEvent_t> sr_evfree;
    hipGraphExec_t sr_graph = nullptr;  // SR_GRAPH_ITERS iterations from parity 0
};

// Helpers shared by the host units: hidden, so the library exports only the C-ABI
// (and the kernels).
namespace gkh __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;  // gk_last_error's text (gk_api.hip)
int set_err(int code, const char *fmt, ...);

#define HIPCHK(call)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return set_err(GK_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #call, \
                                             hipGetErrorString(e_));                            \
    } while (0)
#define NCCLCHK(call)                                                                           \
    do {                                                                                        \
        ncclResult_t r_ = (call);                                                               \
        if (r_ != ncclSuccess) return set_err(GK_ERR_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #call, \
                                              ncclGetErrorString(r_));                          \
    } while (0)
#define CHK(call)                      \
    do {                               \
        int s_ = (call);               \
        if (s_ != GK_OK) return s_;    \
    } while (0)
#define LAUNCHCHK() HIPCHK(hipGetLastError())

constexpr int NSLOT = 4;  // partial slabs (ping-pong + spares)
constexpr int PROF_POOL = 8192;

// gk_api.hip
int prof_harvest(gk_ctx *c);
void graph_reset(gk_ctx *c);
void set_geometry(gk_grid *g);
int check_ctx(gk_ctx *c);
// ... and the range checks of the step and the update / v_err entries
inline int check_step(const gk_ctx *c, int j) {
    return j < 1 || j > c->m ? set_err(GK_ERR_ARG, "step j=%d outside 1..%d", j, c->m) : GK_OK;
}
inline int check_nout(const gk_ctx *c, int n_out) {
    return n_out < 1 || n_out > c->m ? set_err(GK_ERR_ARG, "bad n_out %d", n_out) : GK_OK;
}
// The short-recurrence solvers keep their vectors in the Krylov columns and their
// state on the device: any call that changes the operator data, the right-hand
// side or x, or that starts a GMRES cycle (which overwrites the columns), ends the
// running gk_sr_* solve -- later gk_sr_iterate / status / history refuse until the
// next gk_sr_start.
inline void sr_invalidate(gk_ctx *c) { c->sr_solver = -1; }
// The diagonal of the grid's operator A_poisson + shift I, the `diag` every stencil-carrying
// kernel takes: fl(4 + shift), rounded once here and never in a kernel.
inline double diag_of(const gk_grid *g) { return 4.0 + g->shift; }
// The context's side: the MGS-R cycle's.  The short-recurrence solvers and Householder's
// GK_HH_PREC_LEFT precondition on the left only; GK_HH_PREC_RIGHT does not ask the context.
inline bool right_prec(const gk_ctx *c) { return c->side == GK_SIDE_RIGHT && c->pkind != GK_PREC_IDENTITY; }

// Compressed basis (gk_cb.hpp): the FP32 columns in the lower half of V, the two widened
// FP64 vectors the operator stage reads in its last two double columns.
inline bool cb_on(const gk_ctx *c) { return c->basis == GK_BASIS_F32; }
// The MGS-R cycle steps by CGS2 (gk_set_orthogonalization; FP64 columns only, gk_cgs.hpp)
inline bool cgs_on(const gk_ctx *c) { return c->orth == GK_ORTH_CGS2; }
template <class T>  // column k (0-based) of the MGS-R basis in the type T it is stored in
inline T *vcol(const gk_ctx *c, int k) { return reinterpret_cast<T *>(c->V) + (i64)k * c->ld; }
inline double *cb_v1w(const gk_ctx *c) { return c->V + (i64)(c->m - 1) * c->ld; }
inline double *cb_vjw(const gk_ctx *c) { return c->V + (i64)c->m * c->ld; }
// The Krylov columns by non-temporal loads (GK_TUNE_PROJ_NT; auto: set_geometry's nt_auto)
inline bool nt_cols(const gk_grid *g) { return g->tune_nt > 0 || (g->tune_nt < 0 && g->nt_auto); }
// H(1:j+1, j) of step j: its device slot, the mapped mirror the step's last kernel publishes
// it to (the device's address of it) and the host's view of that mirror
struct HCol { double *dev, *map; const volatile double *host; };
inline HCol hcol_of(const gk_ctx *c, int j) {
    const i64 off = (i64)(j - 1) * (c->m + 2);
    return {c->hall + off, c->hallh_dev + off, c->hallh + off};
}

// gk_op.hip -- the operator A, the preconditioner M and their products.  acc: the reduction
// fused into the launch that writes `out` (gk::ACC_*; ACC_DOT with vdot), its partials in
// `part`, their count in last_np.  Every one exchanges the halos of what it reads.  What takes
// a gk_grid * runs on a bare grid too; a multigrid preconditioner needs the context.
int op_A(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part);
int op_resid(gk_ctx *c, const double *x, double *out, int acc, double *part);  // out = b - A x
int stencil_plain_raw(gk_grid *g, const double *x, const double *hlo, const double *hhi, double *y);
int grid_sweeps(gk_grid *g, const double *in, double *out, int acc, const double *vdot, double *part);
int precond_sweeps(gk_ctx *c, const double *in, double *out, int acc, const double *vdot, double *part);
int grid_Minv_or_copy(gk_grid *g, const double *in, double *out);
int op_Minv_or_copy(gk_ctx *c, const double *in, double *out);
int op_precond(gk_ctx *c, const double *v, double *out, bool resid, int acc, const double *vdot, double *part);
int op_right(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part);
int add_precond(gk_ctx *c, const double *t);         // x += M^-1 t, one march where cbpr2 allows
int add_precond_sweeps(gk_ctx *c, const double *t);  // ... always the sweeps into z, then add_into
// GK_PREC_MG: the hierarchy of a whole-grid single-rank context (built by gk_set_precond, freed
// by it and by gk_destroy), the V-cycle behind precond_sweeps, and gk_mg_transfer's launches
int mg_build(gk_ctx *c, double p0, double p1, int degree);
void mg_refresh(gk_ctx *c);  // the levels' shift, intervals and coarsest degree from c->shift (no allocation)
void mg_free(gk_ctx *c);
int mg_apply(gk_ctx *c, const double *in, double *out, int acc, const double *vdot, double *part);
int mg_transfer(gk_ctx *c, int what, int level, const double *a, const double *b, double *out);

// gk_step.hip -- what every Arnoldi path launches, and the MGS-R cycle.  proj: one k_proj
// launch on double columns (mode: gk::PJ_*; the float-column form stays inside the unit).
int proj(gk_grid *g, int mode, double *w, const double *va, const double *vb, const double *pin, int npin,
         double *pout, double *hslot, double coef, i64 tail0 = 0, int hstore = 0);
int scale(gk_ctx *c, double *out, const double *w, const double *pin, int npin, double *hslot,
          double *hcopy = nullptr, const double *hsrc = nullptr, int ncopy = 0, bool pin_norm = false);
int add_into(gk_ctx *c, double *x, const double *w);  // x += w (k_add, GK_KID_UPDATE)
int fill_hash(gk_ctx *c, double *x, unsigned long long seed);  // k_fill_hash of the global index
int finalize(gk_grid *g, const double *pin, int npin, double *out, int take_sqrt);
bool res_plan(gk_ctx *c, gk::ResPlan &p, bool hh = false);
enum { RESF_CLOSE_HH = 1, RESF_UNIT_INIT = 2, RESF_PIN_LOCAL = 4 };  // res_step's flags
int res_step(gk_ctx *c, int j, const gk::ResPlan &p, const double *pin, int npin, double *hs, double *hcopy,
             int mode = gk::RES_MGS, double *w = nullptr, i64 unit_g = -1, int flags = 0);
bool cb_plan_ctx(gk_ctx *c, gk::CbPlan &p);
int d2h_sync(gk_ctx *c, double *host, const double *dev, int count);
bool verr_ref_order(const gk_ctx *c);
int ensure_gram(gk_ctx *c, int ncols);
int gram(gk_ctx *c, const double *base, int ncols, std::vector<double> &G);
int update_begin(gk_ctx *c, const double *y, int n_out);  // gk_update_x / gk_hh_update_x: checks, y to ydev

// gk_comm.hip
bool collective(const gk_grid *g);  // false on a bare grid
void xs_set_timeout(gk_ctx *c, int ms);
int xs_check(gk_ctx *c);
int res_check(gk_ctx *c);
int spin_until(gk_ctx *c, hipError_t (*query)(void *), void *obj, const char *what);
hipError_t query_stream(void *s);
hipError_t query_event(void *e);
int sync_st(gk_ctx *c);
// The tail of an entry that returns with its work done: the stream drained, then the profiling events
inline int sync_harvest(gk_ctx *c) {
    const int s = sync_st(c);
    return s == GK_OK && c->prof ? prof_harvest(c) : s;
}
int allreduce(gk_ctx *c, double *buf, int count, bool vec = false);
int bcast(gk_ctx *c, double *buf, int count, int root);
int halo_lines(gk_grid *g, const double *vec, int nl, double *lo, double *hi);
int halo(gk_grid *g, const double *vec);
const double *halo_lo(const gk_grid *g);
const double *halo_hi(const gk_grid *g);

struct ProfScope {
    gk_ctx *c;
    int slot = -1;
    ProfScope(gk_grid *g, int kid) : c(g->ctx) {
        if (c == nullptr || !c->prof || !c->prof_on_step || c->capturing) return;
        if (c->nev == PROF_POOL) prof_harvest(c);
        slot = c->nev++;
        c->evk[slot] = kid;
        (void)hipEventRecord(c->ev0[slot], c->st);
    }
    ~ProfScope() {
        if (slot >= 0) (void)hipEventRecord(c->ev1[slot], c->st);
    }
};

inline double *slot(const gk_grid *g, int s) { return g->red + (i64)s * gk::NPMAX; }

}  // namespace gkh
