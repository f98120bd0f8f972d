// gk_op.hip -- the operator and the preconditioner as the solvers apply them: A v,
// b - A x, M^-1 v, M^-1 A v, A M^-1 v and x += M^-1 t.  What A is and how it is launched
// is known here and in gk_stencil.hpp (this unit alone includes it, and alone calls
// gk::cheb_launch); the fused device paths of gk_cheb.hpp and gk_sr.hpp embody the same
// operator.  The multigrid preconditioner (GK_PREC_MG) is a composition of these launches
// per level with gk_mg.hpp's transfers.  Declarations: gk_host.hpp.
#include <algorithm>
#include <cmath>

#include "gk_cheb.hpp"
#include "gk_host.hpp"
#include "gk_mg.hpp"
#include "gk_stencil.hpp"

namespace gkh __attribute__((visibility("hidden"))) {

// -------------------------------------------------------------- launches ---
template <int VEC, int OP, int ACC>
int launch_stencil_v(gk_grid *c, const gk::StArgs &a) {
    gk::k_stencil<VEC, OP, ACC><<<c->sgrid, gk::TPB, 0, c->st>>>(a);
    LAUNCHCHK();
    return GK_OK;
}

template <int OP, int ACC>
int launch_stencil_o(gk_grid *c, const gk::StArgs &a) {
    return c->vec == 2 ? launch_stencil_v<2, OP, ACC>(c, a) : launch_stencil_v<1, OP, ACC>(c, a);
}

template <int OP>
int launch_stencil_a(gk_grid *c, int acc, const gk::StArgs &a) {
    if (acc == gk::ACC_NONE) return launch_stencil_o<OP, gk::ACC_NONE>(c, a);
    if (acc == gk::ACC_DOT) return launch_stencil_o<OP, gk::ACC_DOT>(c, a);
    return launch_stencil_o<OP, gk::ACC_NORM>(c, a);
}

// One sweep on the grid's slab, its halo lines already exchanged (halo(c, a.x)).
int stencil(gk_grid *c, int op, int acc, gk::StArgs a) {
    ProfScope ps(c, GK_KID_STENCIL);
    if (acc != gk::ACC_NONE) c->last_np = c->np_st;
    a.hlo = halo_lo(c);
    a.hhi = halo_hi(c);
    a.diag = diag_of(c);
    a.N = c->N;
    a.nlines = c->nlines;
    a.JT = c->JT;
    switch (op) {
        case gk::OP_PLAIN: return launch_stencil_a<gk::OP_PLAIN>(c, acc, a);
        case gk::OP_RESID: return launch_stencil_a<gk::OP_RESID>(c, acc, a);
        case gk::OP_CBPR2: return launch_stencil_a<gk::OP_CBPR2>(c, acc, a);
        case gk::OP_CHEB_FIRST: return launch_stencil_a<gk::OP_CHEB_FIRST>(c, acc, a);
        case gk::OP_CBPR2_ADD:  // the update's accumulate form carries no reduction
            if (acc != gk::ACC_NONE) return set_err(GK_ERR_ARG, "OP_CBPR2_ADD: reduction %d", acc);
            return launch_stencil_o<gk::OP_CBPR2_ADD, gk::ACC_NONE>(c, a);
        default: return launch_stencil_a<gk::OP_CHEB_ITER>(c, acc, a);
    }
}

// out = A v with the fused reduction `acc` (none, the dot with vdot, or the norm) in slab
// `part` (np_st partials)
int op_A(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part) {
    CHK(halo(c, v));
    gk::StArgs a{};
    a.x = v;
    a.y = out;
    a.vdot = vdot;
    a.part = part;
    return stencil(c, gk::OP_PLAIN, acc, a);
}

// out = b - A x, likewise (the cycle starts take the norm)
int op_resid(gk_ctx *c, const double *x, double *out, int acc, double *part) {
    if (acc == gk::ACC_DOT) return set_err(GK_ERR_ARG, "op_resid: no dot partner");
    CHK(halo(c, x));
    gk::StArgs a{};
    a.x = x;
    a.in1 = c->b;
    a.y = out;
    a.part = part;
    return stencil(c, gk::OP_RESID, acc, a);
}

// y = A x on a slab whose neighbour lines the caller holds (nullptr: physical boundary):
// no communicator, no profiling scope -- gk_poisson5's bare grid.
int stencil_plain_raw(gk_grid *c, const double *x, const double *hlo, const double *hhi, double *y) {
    gk::StArgs a{};
    a.x = x;
    a.y = y;
    a.diag = diag_of(c);
    a.N = c->N;
    a.nlines = c->nlines;
    a.JT = c->JT;
    a.hlo = hlo;
    a.hhi = hhi;
    return launch_stencil_o<gk::OP_PLAIN, gk::ACC_NONE>(c, a);
}

// cbpr2 coefficients exactly as chebyshev.f90:19-25
void cbpr2_coefs(const gk_grid *c, double *d_out, double *alpha_out) {
    const double em = c->p0, eM = c->p1;
    const double cc = (eM - em) / 2.0;
    const double d = (eM + em) / 2.0;
    double alpha = 1.0 / d;
    double beta = cc * alpha / 2.0;
    beta = beta * beta;
    alpha = 1.0 / (d - beta);
    *d_out = d;
    *alpha_out = alpha;
}

// The one-launch route of w = A (M^-1 v) (gk::k_right_cbpr2): cbpr2 on one rank
// that holds the whole grid -- the march has no halo lines, the level-1 value of a
// neighbour's line would need two of its lines.  Everything else takes the
// two-launch route (GK_TUNE_RIGHT_FUSED 0 forces it).
bool right_fused_ok(const gk_ctx *c) {
    return c->tune_right_fused != 0 && c->pkind == GK_PREC_CBPR2 && c->nranks == 1 && c->line0 == 0 &&
           c->nlines == c->N;
}

template <int VEC>
int launch_right_v(gk_ctx *c, int acc, const gk::RcArgs &a) {
    if (acc == gk::ACC_DOT)
        gk::k_right_cbpr2<VEC, gk::ACC_DOT><<<c->sgrid, gk::TPB, 0, c->st>>>(a);
    else
        gk::k_right_cbpr2<VEC, gk::ACC_NONE><<<c->sgrid, gk::TPB, 0, c->st>>>(a);
    LAUNCHCHK();
    return GK_OK;
}

// out = A (cbpr2 v) in one launch; acc = ACC_DOT leaves <out, vdot> in slab `part`
// (np_st partials, k_stencil's layout).
int right_cbpr2(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part) {
    if (acc != gk::ACC_NONE && acc != gk::ACC_DOT) return set_err(GK_ERR_ARG, "right_cbpr2: reduction %d", acc);
    ProfScope ps(c, GK_KID_STENCIL);
    if (acc != gk::ACC_NONE) c->last_np = c->np_st;
    gk::RcArgs a{};
    a.v = v;
    a.w = out;
    a.vdot = vdot;
    a.part = part;
    cbpr2_coefs(c, &a.d, &a.alpha);
    a.diag = diag_of(c);
    a.N = c->N;
    a.nlines = c->nlines;
    a.JT = c->JT;
    return c->vec == 2 ? launch_right_v<2>(c, acc, a) : launch_right_v<1>(c, acc, a);
}

// One temporal-blocked pass (gk_cheb.hip), tiles sized by the largest slab so
// every rank writes the same number of partials (the all-reduced slab has one
// length on all ranks).
int launch_cf(gk_grid *c, int L, bool first, bool last, int acc, gk::CFArgs &a, i64 *np, bool sten = false) {
    gk::CFLaunch q{};
    q.L = L;
    q.sten = sten;
    q.first = first;
    q.last = last;
    q.acc = acc;
    q.lines = (c->ctx != nullptr && c->ctx->nranks > 1 && c->max_lines > c->nlines) ? c->max_lines : c->nlines;
    q.cus = c->res_cus > 0 ? c->res_cus : 256;
    q.dev = c->dev;
    q.st = c->st;
    const int e = gk::cheb_launch(q, a, np);
    if (e == gk::GK_CF_ESLOT) return set_err(GK_ERR_ARG, "Chebyshev pass grid exceeds a reduction slot");
    if (e == gk::GK_CF_ESTEN) return set_err(GK_ERR_ARG, "fused-stencil Chebyshev pass outside its variants");
    if (e == gk::GK_CF_ESPILL)
        return set_err(GK_ERR_HIP, "Chebyshev pass (L = %d) was built with a register spill to scratch; refused", L);
    if (e != 0) return set_err(GK_ERR_HIP, "Chebyshev pass launch: %s", hipGetErrorString((hipError_t)e));
    return GK_OK;
}

// Chebyshev(k <= 16) as one or two temporal-blocked passes (gk_cheb.hip):
// sweeps 1..min(k, 8) in the first, the rest in the second.  The input is `in`, or
// with sten_v the vector whose stencil image stage 0 forms.
int cheb_fused(gk_grid *c, const double *in, double *out, int acc, const double *vdot, double *part,
               const double *c1, const double *c2, double theta, const double *sten_v) {
    ProfScope ps(c, GK_KID_PREC);
    const int k = c->pdeg;
    const int g1 = std::min(k, gk::CF_LMAX), g2 = k - g1;
    const bool sten = sten_v != nullptr;  // one pass (k <= 8) taking v, stage 0 = the stencil
    // On slabs every input of a pass brings L lines of each neighbour (deep halo).
    const gk_ctx *cx = c->ctx;  // the slabs' context (a bare grid is never one of several)
    const bool slabs = collective(c) && cx->nranks > 1;
    const bool has_lo = slabs && cx->rank > 0, has_hi = slabs && cx->rank < cx->nranks - 1;
    auto dlo = [&](int v) { return cx->dh + (i64)(2 * v) * gk::CF_HMAX * c->N; };
    auto dhi = [&](int v) { return cx->dh + (i64)(2 * v + 1) * gk::CF_HMAX * c->N; };
    auto deep = [&](gk::CFArgs &x, int v, const double *vec, int L) -> int {
        if (slabs) CHK(halo_lines(c, vec, L, dlo(v), dhi(v)));
        x.lo[v] = has_lo ? dlo(v) : nullptr;
        x.hi[v] = has_hi ? dhi(v) : nullptr;
        return GK_OK;
    };
    gk::CFArgs a{};
    a.N = c->N;
    a.nlines = c->nlines;
    a.theta = theta;
    a.diag = diag_of(c);
    a.din = sten ? sten_v : in;
    a.vdot = vdot;
    a.part = part;
    CHK(deep(a, 0, a.din, g1 + (sten ? 1 : 0)));
    for (int l = 0; l < g1; ++l) {
        a.c1[l] = c1[l];
        a.c2[l] = c2[l];
    }
    i64 np = 0;
    if (g2 == 0) {
        a.out = out;
        CHK(launch_cf(c, g1, true, true, acc, a, &np, sten));
        if (acc != gk::ACC_NONE) c->last_np = (int)np;
        return GK_OK;
    }
    a.dout = c->dA;
    a.rout = c->aux;
    a.zout = c->dB;
    CHK(launch_cf(c, g1, true, false, gk::ACC_NONE, a, nullptr));
    gk::CFArgs b{};
    b.N = c->N;
    b.nlines = c->nlines;
    b.diag = diag_of(c);
    b.din = c->dA;
    b.rin = c->aux;
    b.zin = c->dB;
    CHK(deep(b, 0, c->dA, g2));
    CHK(deep(b, 1, c->aux, g2));
    CHK(deep(b, 2, c->dB, g2));
    b.out = out;
    b.vdot = vdot;
    b.part = part;
    for (int l = 0; l < g2; ++l) {
        b.c1[l] = c1[g1 + l];
        b.c2[l] = c2[g1 + l];
    }
    CHK(launch_cf(c, g2, false, true, acc, b, &np));
    if (acc != gk::ACC_NONE) c->last_np = (int)np;
    return GK_OK;
}

// The smallest slab of any rank, gathered once per communicator (collective:
// every rank reaches it at the same point, the first Chebyshev application):
// each rank contributes its nlines at its own position of a short vector that
// is all-reduced by sum.  The decomposition may be any set of consecutive
// slabs (gk_create / gk_comm_init take any line0, nlines), not only
// slab_partition's.
int ensure_min_lines(gk_ctx *c) {
    if (c->min_lines > 0) return GK_OK;
    std::vector<double> v(c->nranks, 0.0);
    v[c->rank] = c->nlines;
    double *d = slot(c, 3);
    HIPCHK(hipMemcpyAsync(d, v.data(), sizeof(double) * c->nranks, hipMemcpyHostToDevice, c->st));
    CHK(allreduce(c, d, c->nranks, true));
    HIPCHK(hipMemcpyAsync(v.data(), d, sizeof(double) * c->nranks, hipMemcpyDeviceToHost, c->st));
    CHK(sync_st(c));
    int mn = c->nlines;
    for (double x : v) mn = std::min(mn, (int)x);
    c->min_lines = mn;
    return GK_OK;
}

// Temporal-blocked Chebyshev passes: even N (two points per lane), k <= 16,
// slabs below 2 GiB per vector, and on slabs every rank holding at least the
// pass's L lines (the deep halo comes from the immediate neighbour only).  The
// same answer on every rank.
int cheb_fused_ok(gk_grid *c, bool *ok) {
    *ok = false;
    if (!c->tune_cheb_fused || c->N % 2 != 0 || c->pdeg > 2 * gk::CF_LMAX) return GK_OK;
    // the pass addresses slab vectors through 32-bit buffer offsets
    if ((i64)c->N * std::max(c->nlines, c->max_lines) * 8 >= (1LL << 31)) return GK_OK;
    if (!collective(c) || c->ctx->nranks == 1) {
        *ok = true;
        return GK_OK;
    }
    CHK(ensure_min_lines(c->ctx));
    *ok = c->ctx->min_lines >= std::min(c->pdeg, gk::CF_LMAX);
    return GK_OK;
}

// Chebyshev(k) coefficients of the sweeps (the per-sweep kernels' recurrence), k each.
constexpr int CHEB_KMAX = 64;  // gk_set_precond's bound on the degree
void cheb_coefs(const gk_grid *c, double *c1, double *c2, double *theta) {
    *theta = (c->p0 + c->p1) / 2.0;
    const double delta = std::fabs(c->p1 - c->p0) / 2.0;
    const double sigma = *theta / delta;
    double rho0 = delta / *theta;
    for (int it = 0; it < c->pdeg; ++it) {
        const double rho1 = 1.0 / (2.0 * sigma - rho0);
        c1[it] = rho1 * rho0;
        c2[it] = 2.0 * rho1 / delta;
        rho0 = rho1;
    }
}

// ------------------------------------------------ multigrid (GK_PREC_MG) ---
// Aggregation multigrid on 2 x 2 blocks: with piecewise-constant P and the 4-member sum
// P^T, P^T A_N P = 2 A_{N/2} -- every level runs the unscaled stencil on a smaller square
// grid, so a level is a bare gk_grid (its side, set_geometry, a Chebyshev smoother) that
// stencil() and grid_sweeps() run on unchanged, and the cycle is a composition of them
// with gk_mg.hpp's three streaming launches.
void mg_free(gk_ctx *c) {
    c->mg.clear();
    if (c->mg_buf != nullptr) {  // queued cycles may still read it
        if (c->st != nullptr) (void)hipStreamSynchronize(c->st);
        (void)hipFree(c->mg_buf);
    }
    c->mg_buf = nullptr;
    c->mg_cdeg = 0;
}

int mg_build(gk_ctx *c, double p0, double p1, int degree) {
    mg_free(c);
    int sides[gk::MG_LMAX];
    const int nl = gk::mg_levels(c->N, sides);
    if (nl < 2) return set_err(GK_ERR_ARG, "multigrid needs an even N with N / 2 >= %d (N = %d)", gk::MG_NMIN, c->N);
    const int L = nl - 1;
    auto vlen = [](int n) { return ((i64)n * n + 31) / 32 * 32; };  // 256-byte aligned vectors
    // level 0: z, t, d; between: r, e, z, t, d and the sweeps' aux, dA, dB; coarsest: r, e, aux, dA, dB
    i64 total = 0;
    for (int l = 0; l <= L; ++l) total += vlen(sides[l]) * (l == 0 ? 3 : (l < L ? 8 : 5));
    HIPCHK(hipSetDevice(c->dev));
    if (hipMalloc(&c->mg_buf, sizeof(double) * (size_t)total) != hipSuccess) {
        c->mg_buf = nullptr;
        return set_err(GK_ERR_NOMEM, "cannot allocate the multigrid hierarchy: %.2f GB", total * 8 / 1e9);
    }
    // zeroed once: every vector is written before the cycle reads it, but never an uninitialised byte
    if (hipMemsetAsync(c->mg_buf, 0, sizeof(double) * (size_t)total, c->st) != hipSuccess) {
        mg_free(c);
        return set_err(GK_ERR_HIP, "memset failed");
    }
    c->mg_p0 = p0;
    c->mg_p1 = p1;
    c->mg_deg = degree;
    double *p = c->mg_buf;
    auto take = [&](int n) {
        double *q = p;
        p += vlen(n);
        return q;
    };
    c->mg.resize(nl);
    for (int l = 0; l <= L; ++l) {
        gk_mg_level &lv = c->mg[l];
        const int n = sides[l];
        gk_grid *gr = &lv.g;  // its block-count tunings stay at their defaults, whatever the parent's
        gr->dev = c->dev;
        gr->N = n;
        gr->nlines = n;
        gr->max_lines = n;
        gr->nloc = (i64)n * n;
        gr->ld = vlen(n);
        gr->st = c->st;
        gr->red = c->red;
        gr->scal = c->scal;
        gr->res_cus = c->res_cus;
        set_geometry(gr);
        gr->pkind = GK_PREC_CHEB;
        if (l > 0) {
            lv.r = take(n);
            lv.e = take(n);
        }
        if (l < L) {
            lv.z = take(n);
            lv.t = take(n);
            lv.d = take(n);
        }
        if (l == 0) {
            gr->aux = c->aux;
            gr->dA = c->dA;
            gr->dB = c->dB;
        } else {
            gr->aux = take(n);
            gr->dA = take(n);
            gr->dB = take(n);
        }
    }
    mg_refresh(c);
    return GK_OK;
}

// The levels under the context's shift sigma.  Every level runs the same unscaled stencil on
// a mesh twice as wide, so the shift is rediscretised by the same scaling, exactly:
// sigma_l = 4^l sigma, diag_l = fl(4 + sigma_l).  (Galerkin: P^T (A + sigma I) P = 2 A_c +
// 4 sigma I; halving it as for A would leave 2 sigma and over-correct the smooth modes.)
// The caller's interval is level 0's; level l smooths on it moved by sigma_l - sigma, the
// coarsest level on its exact interval plus sigma_L with the degree that interval asks for.
// Host state only: captured graphs hold the old values (gk_set_shift drops them).
void mg_refresh(gk_ctx *c) {
    if (c->mg.size() < 2) return;
    const int L = (int)c->mg.size() - 1;
    double sl = c->shift;
    for (int l = 0; l <= L; ++l, sl *= 4.0) {
        gk_grid *gr = &c->mg[l].g;
        gr->shift = sl;
        if (l < L) {
            gr->p0 = c->mg_p0 + (sl - c->shift);
            gr->p1 = c->mg_p1 + (sl - c->shift);
            gr->pdeg = c->mg_deg;
        } else {
            c->mg_cdeg = gk::mg_coarse_degree(gr->N, sl, &gr->p0, &gr->p1);
            gr->pdeg = c->mg_cdeg;
        }
    }
}

// out = r - A z on level grid gr (OP_RESID's expression with in1 = r)
static int mg_resid(gk_grid *gr, const double *z, const double *r, double *out) {
    gk::StArgs a{};
    a.x = z;
    a.in1 = r;
    a.y = out;
    return stencil(gr, gk::OP_RESID, gk::ACC_NONE, a);
}

// rc = P^T (r - A z): one march (GK_TUNE_MG_FUSED), or OP_RESID into t and the plain
// restriction -- the same expressions in the same order, bit-identical rc.
static int mg_resid_restrict(gk_ctx *c, gk_mg_level &lv, const double *r, double *rc) {
    if (c->tune_mg_fused) {
        HIPCHK(gk::mg_restrict(true, lv.g.N, diag_of(&lv.g), lv.z, r, rc, c->st));
        return GK_OK;
    }
    CHK(mg_resid(&lv.g, lv.z, r, lv.t));
    HIPCHK(gk::mg_restrict(false, lv.g.N, 0.0, lv.t, nullptr, rc, c->st));
    return GK_OK;
}

// out = MG_0(in): the V-cycle.  Launches on the context's stream only (no allocation, no
// host synchronisation, no copies), so captured iterations and profiling scopes hold; the
// closing add of level 0 carries the reduction `acc`.  in and out are none of the
// hierarchy's vectors nor aux, dA, dB (precond_sweeps' rule).
int mg_apply(gk_ctx *c, const double *in, double *out, int acc, const double *vdot, double *part) {
    if (c->mg.size() < 2) return set_err(GK_ERR_STATE, "multigrid hierarchy not built");
    ProfScope ps(c, GK_KID_PREC);
    const int L = (int)c->mg.size() - 1;
    for (gk_mg_level &lv : c->mg) lv.g.tune_cheb_fused = c->tune_cheb_fused;  // the smoothers follow the parent's route
    for (int l = 0; l < L; ++l) {  // pre-smoothing from zero, residual, restriction
        gk_mg_level &lv = c->mg[l];
        const double *r = l == 0 ? in : lv.r;
        CHK(grid_sweeps(&lv.g, r, lv.z, gk::ACC_NONE, nullptr, nullptr));
        CHK(mg_resid_restrict(c, lv, r, c->mg[l + 1].r));
    }
    CHK(grid_sweeps(&c->mg[L].g, c->mg[L].r, c->mg[L].e, gk::ACC_NONE, nullptr, nullptr));
    for (int l = L - 1; l >= 0; --l) {  // correction, post-smoothing on the new residual
        gk_mg_level &lv = c->mg[l];
        gk_grid *gr = &lv.g;
        const double *r = l == 0 ? in : lv.r;
        HIPCHK(gk::mg_prolong_add(gr->N, lv.z, c->mg[l + 1].e, lv.z, c->st));
        CHK(mg_resid(gr, lv.z, r, lv.t));
        CHK(grid_sweeps(gr, lv.t, lv.d, gk::ACC_NONE, nullptr, nullptr));
        HIPCHK(gk::mg_add(l == 0 ? acc : gk::ACC_NONE, gr->nblk_stream, gr->nloc, lv.z, lv.d, l == 0 ? out : lv.e,
                          vdot, part, c->st));
    }
    if (acc != gk::ACC_NONE) c->last_np = c->mg[0].g.nblk_stream;
    return GK_OK;
}

// gk_mg_transfer's launches between level `level` and the next, host arrays staged through
// the hierarchy's own vectors.
int mg_transfer(gk_ctx *c, int what, int level, const double *a, const double *b, double *out) {
    gk_mg_level &f = c->mg[level], &g = c->mg[level + 1];
    const int N = f.g.N;
    const size_t nf = sizeof(double) * (size_t)f.g.nloc, nc = sizeof(double) * (size_t)g.g.nloc;
    if (what == 2) {  // out = a + P b, in place as the cycle runs it
        HIPCHK(hipMemcpyAsync(f.z, a, nf, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(g.e, b, nc, hipMemcpyHostToDevice, c->st));
        HIPCHK(gk::mg_prolong_add(N, f.z, g.e, f.z, c->st));
        HIPCHK(hipMemcpyAsync(out, f.z, nf, hipMemcpyDeviceToHost, c->st));
        return sync_st(c);
    }
    HIPCHK(hipMemcpyAsync(f.t, a, nf, hipMemcpyHostToDevice, c->st));
    if (what == 1) {  // out = P^T (a - A b) by the fused march
        HIPCHK(hipMemcpyAsync(f.z, b, nf, hipMemcpyHostToDevice, c->st));
        HIPCHK(gk::mg_restrict(true, N, diag_of(&f.g), f.z, f.t, g.r, c->st));
    } else {  // out = P^T a
        HIPCHK(gk::mg_restrict(false, N, 0.0, f.t, nullptr, g.r, c->st));
    }
    HIPCHK(hipMemcpyAsync(out, g.r, nc, hipMemcpyDeviceToHost, c->st));
    return sync_st(c);
}

// out = M^-1 in by cbpr2 or the Chebyshev sweeps; `in` is read in place (in != out, and for
// Chebyshev neither is one of the sweeps' work vectors aux, dA, dB).
int grid_sweeps(gk_grid *c, const double *in, double *out, int acc, const double *vdot, double *part) {
    bool fused = false;
    if (c->pkind == GK_PREC_CHEB) CHK(cheb_fused_ok(c, &fused));
    if (!fused) CHK(halo(c, in));  // the fused passes bring their own deep halos
    if (c->pkind == GK_PREC_CBPR2) {
        double d, alpha;
        cbpr2_coefs(c, &d, &alpha);
        gk::StArgs b2{};
        b2.x = in;
        b2.y = out;
        b2.vdot = vdot;
        b2.part = part;
        b2.s1 = d;
        b2.s2 = alpha;
        return stencil(c, gk::OP_CBPR2, acc, b2);
    }
    double c1[CHEB_KMAX], c2[CHEB_KMAX], theta;
    cheb_coefs(c, c1, c2, &theta);
    if (fused) return cheb_fused(c, in, out, acc, vdot, part, c1, c2, theta, nullptr);
    // Chebyshev(k): k sweeps, each one stencil on d_k fused with the three
    // vector updates (res, d, z); the first sweep builds d_0 = r/theta on load.
    double *dcur = c->dA, *dnext = c->dB;
    for (int it = 0; it < c->pdeg; ++it) {
        const bool last = (it == c->pdeg - 1);
        gk::StArgs s{};
        s.y = out;
        s.s2 = c1[it];
        s.s3 = c2[it];
        s.vdot = vdot;
        s.part = part;
        if (it == 0) {
            s.x = in;
            s.s1 = theta;
            s.o_res = last ? nullptr : c->aux;
            s.o_d = last ? nullptr : dcur;
            CHK(stencil(c, gk::OP_CHEB_FIRST, last ? acc : gk::ACC_NONE, s));
        } else {
            CHK(halo(c, dcur));
            s.x = dcur;
            s.in1 = c->aux;
            s.in2 = out;
            s.o_res = last ? nullptr : c->aux;
            s.o_d = last ? nullptr : dnext;
            CHK(stencil(c, gk::OP_CHEB_ITER, last ? acc : gk::ACC_NONE, s));
            std::swap(dcur, dnext);
        }
    }
    return GK_OK;
}

// ... or the multigrid cycle, which is the context's (the same rule for its vectors)
int precond_sweeps(gk_ctx *c, const double *in, double *out, int acc, const double *vdot, double *part) {
    return c->pkind == GK_PREC_MG ? mg_apply(c, in, out, acc, vdot, part) : grid_sweeps(c, in, out, acc, vdot, part);
}

// out = M^-1 in where M may be the identity (then a device copy)
int grid_Minv_or_copy(gk_grid *c, const double *in, double *out) {
    if (c->pkind != GK_PREC_IDENTITY) return grid_sweeps(c, in, out, gk::ACC_NONE, nullptr, nullptr);
    HIPCHK(hipMemcpyAsync(out, in, sizeof(double) * c->nloc, hipMemcpyDeviceToDevice, c->st));
    return GK_OK;
}
int op_Minv_or_copy(gk_ctx *c, const double *in, double *out) {
    return c->pkind == GK_PREC_MG ? mg_apply(c, in, out, gk::ACC_NONE, nullptr, nullptr) : grid_Minv_or_copy(c, in, out);
}

// The Arnoldi step's out = M^-1 (A v) with Chebyshev(k <= 8) as ONE pass whose
// stage 0 forms z = A v itself: no stencil launch, no z vector (the pass reads
// v; on slabs v brings k + 1 deep-halo lines).  *done = false: not applicable
// (the caller takes the stencil + pass route).
int op_precond_sten(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part,
                    bool *done) {
    *done = false;
    if (c->pkind != GK_PREC_CHEB || acc != gk::ACC_DOT || !c->tune_cheb_sten || c->pdeg > gk::CF_LMAX ||
        c->N < gk::CF_PTS)
        return GK_OK;
    bool fused = false;
    CHK(cheb_fused_ok(c, &fused));
    if (!fused || (collective(c) && c->nranks > 1 && c->min_lines < c->pdeg + 1)) return GK_OK;
    double c1[CHEB_KMAX], c2[CHEB_KMAX], theta;
    cheb_coefs(c, c1, c2, &theta);
    CHK(cheb_fused(c, nullptr, out, acc, vdot, part, c1, c2, theta, v));
    *done = true;
    return GK_OK;
}

// out = M^-1 (A v)  or  out = M^-1 (b - A v) (resid); the LAST sweep carries
// the fused reduction `acc` (dot with vdot, or norm) into slab `part`.
// Reference: gmres_mgsr.f90:336-337 (step), :314-320 (cycle start).
int op_precond(gk_ctx *c, const double *v, double *out, bool resid, int acc, const double *vdot,
               double *part) {
    if (!resid) {
        bool done = false;
        CHK(op_precond_sten(c, v, out, acc, vdot, part, &done));
        if (done) return GK_OK;
    }
    if (c->pkind == GK_PREC_IDENTITY)
        return resid ? op_resid(c, v, out, acc, part) : op_A(c, v, out, acc, vdot, part);
    // z = A v   (or b - A v)
    CHK(resid ? op_resid(c, v, c->z, gk::ACC_NONE, nullptr) : op_A(c, v, c->z, gk::ACC_NONE, nullptr, nullptr));
    return precond_sweeps(c, c->z, out, acc, vdot, part);
}

// out = A (M^-1 v), the right-preconditioned Arnoldi operator (M not the identity),
// with the fused reduction `acc` (none, or the dot with vdot) on the launch that
// writes out.  One launch where k_right_cbpr2 applies; else z = M^-1 v by the
// preconditioner's own route (N ranks: halo of v, the sweeps, halo of z) and the
// plain stencil.
int op_right(gk_ctx *c, const double *v, double *out, int acc, const double *vdot, double *part) {
    if (right_fused_ok(c)) return right_cbpr2(c, v, out, acc, vdot, part);
    CHK(precond_sweeps(c, v, c->z, gk::ACC_NONE, nullptr, nullptr));
    return op_A(c, c->z, out, acc, vdot, part);
}

// x += M^-1 t, the cycle-end update of a right-preconditioned Householder cycle (M not
// the identity; t is not z).  Where k_right_cbpr2 applies, ONE march: the cbpr2 sweep
// with the accumulating output (OP_CBPR2_ADD: t and x read, x written, z never stored).
// Else z = M^-1 t by the preconditioner's own route and k_add -- the same expressions
// in the same order, so x is bit-identical on both routes.
int add_precond(gk_ctx *c, const double *t) {
    if (right_fused_ok(c)) {
        gk::StArgs a{};
        a.x = t;
        a.in1 = c->x;
        a.y = c->x;
        cbpr2_coefs(c, &a.s1, &a.s2);
        return stencil(c, gk::OP_CBPR2_ADD, gk::ACC_NONE, a);
    }
    return add_precond_sweeps(c, t);
}

// ... by the two-launch route alone (the MGS-R update's: it never takes the one march)
int add_precond_sweeps(gk_ctx *c, const double *t) {
    CHK(precond_sweeps(c, t, c->z, gk::ACC_NONE, nullptr, nullptr));
    return add_into(c, c->x, c->z);
}

}  // namespace gkh
