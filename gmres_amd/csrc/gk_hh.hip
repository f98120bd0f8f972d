// gk_hh.hip -- the Householder cycle: gk_hh_cycle_start / step / update_x / verr on
// gk_step.hip's launches (proj, scale, res_step, gram) and its own small kernels
// (gk_hh_kernels.hpp, which this unit alone includes).  Declarations: gk_host.hpp.
#include <algorithm>

#include "gk_hh_kernels.hpp"
#include "gk_host.hpp"
#include "gk_resident.hpp"

using namespace gkh;
using gk::ResPlan;

// Global indices 0 .. m -- all the Householder path moves between ranks: w(1:j+1) -- live on the
// rank whose slab starts at line 0, checked at cycle start (its slab holds m+2 unknowns).
static constexpr int HH_ROOT = 0;

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
    if (c->rank == HH_ROOT)
        HIPCHK(hipMemcpyAsync(c->hb, c->w + (0 - c->g0), sizeof(double) * (j + 1), hipMemcpyDeviceToDevice, c->st));
    return bcast(c, c->hb, j + 1, HH_ROOT);
}

// NORM2 of x(0:n) in flang-rt's order into out[0] (GK_TUNE_HH_NORM_ORDER)
static int norm2_seq(gk_ctx *c, const double *x, i64 n, double *out) {
    ProfScope ps(c, GK_KID_OTHER);
    gk::k_norm2_seq<<<1, gk::TPB, 0, c->st>>>(x, n, out);
    LAUNCHCHK();
    return GK_OK;
}

// v <- P_1 .. P_k v  (apply reflections k..1; hh_step :269-283, update :361-373,
// calculate_verr :581-585).  The chain's first launch is a pure dot.
// unit_g >= 0: v is the unit vector e at global index unit_g (gk_hh_step's v_j,
// calculate_verr's columns), so the chain's leading dot <e, P_k> is the single
// element P_k(unit_g) -- exactly what the full dot sums to -- and the resident
// launch skips that pass.
static int reflect_chain_down(gk_ctx *c, double *v, int k, i64 unit_g = -1, int flags = 0) {
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

// The closing of a cycle start (j = 0; gmres_hh.f90:250-253) and of a step whose chain left
// it to the host (:305-318), from the all-reduced partials of ||w(j+1:n)||^2 (np of them in
// slot s0): the pivot w(1:j+1) to every rank, H(1:j+1, j) (j = 0: g1) to hcol / hcopy, the
// fix-up of w, and P(:,j+1) = w / ||w||.  GK_TUNE_HH_NORM_ORDER takes both norms in the
// reference's order instead.
static int hh_close(gk_ctx *c, int j, int s0, int s1, int np, double *hcol, double *hcopy) {
    const bool seq = hh_seq_norms(c);
    if (seq) {  // tmp = norm2(w(j+1:n)) (j = 0: beta = norm2(w))
        CHK(norm2_seq(c, c->w + j, c->nloc - j, slot(c, s0)));
        np = 1;
    }
    CHK(hh_pivot(c, j));
    {
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_hh_pivot<<<1, gk::TPB, 0, c->st>>>(c->hb, slot(c, s0), np, j, hcol, c->scal + 2, hcopy, seq ? 1 : 0);
        LAUNCHCHK();
        // j = 0: w(1) = sign(beta,w(1)) + w(1); the partials of norm2(w)
        gk::k_hh_fix<<<c->nblk_stream, gk::TPB, 0, c->st>>>(c->w, c->nloc, c->g0, j, j, c->scal + 2, slot(c, s1));
        LAUNCHCHK();
    }
    double *out = c->V + (i64)j * c->ld;
    if (seq) {  // w = w / norm2(w) (:315)
        CHK(norm2_seq(c, c->w, c->nloc, slot(c, s1)));
        return scale(c, out, c->w, slot(c, s1), 1, nullptr, nullptr, nullptr, 0, true);
    }
    CHK(allreduce(c, slot(c, s1), c->nblk_stream));
    return scale(c, out, c->w, slot(c, s1), c->nblk_stream, nullptr);
}

extern "C" {

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
    CHK(hh_close(c, 0, 0, 1, c->last_np, c->hcol, nullptr));
    CHK(d2h_sync(c, g1, c->hcol, 1));
    c->cycle_hh = true;
    c->cycle_mgs = false;
    c->hh_prec = precondition;
    return GK_OK;
}

int gk_hh_step_async(gk_ctx *c, int j, int precondition) {
    CHK(check_ctx(c));
    if (cb_on(c)) return set_err(GK_ERR_STATE, "the FP32 basis is MGS-R only (gk_set_basis_precision)");
    CHK(check_step(c, j));
    if (!c->cycle_hh) return set_err(GK_ERR_STATE, "gk_hh_step before gk_hh_cycle_start");
    CHK(hh_prec_arg(c, precondition));
    if ((precondition == GK_HH_PREC_RIGHT) != (c->hh_prec == GK_HH_PREC_RIGHT))
        return set_err(GK_ERR_STATE, "gk_hh_step with precondition = %d in a cycle started with %d", precondition,
                       c->hh_prec);
    HIPCHK(hipSetDevice(c->dev));
    const i64 ld = c->ld;
    double *P = c->V;
    const HCol h = hcol_of(c, j);
    // The w-only resident variant folds the step's small launches into its chains
    // (GK_TUNE_HH_FUSE): the DOWN chain builds e_j itself (no k_set_unit), the UP
    // chain ends with the fix-up and P(:,j+1) = w/||w|| (no k_hh_fix, no k_scale).
    ResPlan rp;
    const bool res = res_plan(c, rp, true);
    // (reference-order reflector norms: the unfused step)
    const bool fuse = res && rp.wo && c->tune_hh_fuse != 0 && !hh_seq_norms(c);
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
    if (res) {
        // w = P_j .. P_1 w and ||w(j+1:n)||^2 as one resident launch; fused: also the fix-up and
        // P(:,j+1).  N ranks on the device exchange: <w, P_1> summed across ranks inside the
        // launch (GK_TUNE_RES_FOLD)
        const bool fold = c->tune_res_fold && c->xs_on && c->nranks > 1;
        if (!fold) CHK(allreduce(c, slot(c, s0), np));
        CHK(res_step(c, j, rp, slot(c, s0), np, slot(c, s1), nullptr, gk::RES_HH_UP, c->w, -1,
                     (fuse ? RESF_CLOSE_HH : 0) | (fold ? RESF_PIN_LOCAL : 0)));
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
    if (fuse) {  // H(1:j+1, j) from hb (written by the owner rank's launch) on every rank
        CHK(bcast(c, c->hb, j + 1, HH_ROOT));
        ProfScope ps(c, GK_KID_OTHER);
        gk::k_hh_pivot<<<1, gk::TPB, 0, c->st>>>(c->hb, slot(c, s0), np, j, h.dev, c->scal + 2, h.map);
        LAUNCHCHK();
    } else {
        CHK(hh_close(c, j, s0, s1, np, h.dev, h.map));
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
    CHK(update_begin(c, y, n_out));
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
    return sync_harvest(c);
}

int gk_hh_verr(gk_ctx *c, int n_out, double *v_err) {
    CHK(check_ctx(c));
    CHK(check_nout(c, n_out));
    HIPCHK(hipSetDevice(c->dev));
    if (c->Vb == nullptr && hipMalloc(&c->Vb, sizeof(double) * (size_t)c->ld * c->m) != hipSuccess)
        return set_err(GK_ERR_NOMEM, "cannot allocate the verr basis");
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

}  // extern "C"
