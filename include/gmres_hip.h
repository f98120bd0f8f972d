/*
 * gmres_hip.h -- C-ABI of libgmres_hip.so, the MI355X (gfx950) device side of
 * the restarted GMRES(m) inner cycle for the 2D Poisson 5-point operator.
 *
 * Drop-in boundary.  The reference (AlexanderGSC/gmres, Fortran) plugs its
 * operator and preconditioner into the solvers through two abstract
 * interfaces (src/interfaces.f90:13-17 `stencil_vector(x,y,n)` and
 * :20-27 `precond(A_x,r,z,aux,params,n)`), and the solvers
 * (src/gmres_mgsr.f90:277-421 gmres_mgsr_omp, :98-199 gmres_mgsr_mf,
 * src/gmres_hh.f90:211-385 gmres_hh_omp, :388-566 gmres_hh_prec_omp) run the
 * Arnoldi cycle on host arrays.  This library replaces the vector work of
 * those solvers with HIP kernels on device-resident data; the small
 * Hessenberg / Givens / back-solve work stays on the host (Fortran module
 * gmres_amd/fortran/gmres_hip.f90 binds these symbols with ISO_C_BINDING).
 *
 * Conventions
 *   - Every function returns int status: GK_OK (0) or a negative GK_ERR_*;
 *     gk_last_error() returns a message for the calling thread's last error.
 *   - Grid: N x N ("nside"), Fortran column-major, idx = i + (j-1)*N with i
 *     fastest.  A context owns the slab of grid lines j in [line0, line0+nlines)
 *     (0-based line0); nloc = N*nlines local unknowns.  Single GPU:
 *     line0 = 0, nlines = N.
 *   - Host arrays are plain double* of the local length; device pointers in
 *     the stateless kernel API are plain device addresses (16-byte aligned).
 *   - `j` arguments are 1-based Arnoldi step numbers as in the reference.
 *   - A context is single-host-thread, stream-ordered, not re-entrant.
 */
#ifndef GMRES_HIP_H
#define GMRES_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GK_OK 0
#define GK_ERR_ARG (-1)   /* bad argument (shape, range, alignment, order) */
#define GK_ERR_HIP (-2)   /* HIP runtime error */
#define GK_ERR_RCCL (-3)  /* RCCL error */
#define GK_ERR_STATE (-4) /* call out of order (e.g. step before cycle start) */
#define GK_ERR_NOMEM (-5) /* device allocation failed */
#define GK_ERR_COMM (-6)  /* device exchange: a peer missed its deadline (see gk_comm_init_xgmi) */

/* Preconditioner kinds (the reference's `precond` plug-ins). */
#define GK_PREC_IDENTITY 0 /* z = r ; config 1 "no precond"  */
#define GK_PREC_CBPR2 1    /* src/preconds/chebyshev.f90:8-38, params(1:2) */
#define GK_PREC_CHEB 2     /* Chebyshev(k) semi-iteration, build-defined (BASELINE config 3) */
#define GK_PREC_MG 3       /* aggregation multigrid V-cycle, Chebyshev(degree) smoothing (beyond the reference) */

/* Kernel ids for gk_profile_read(). */
#define GK_KID_PROJ 0    /* fused MGS-R / Householder projection (axpy_i + dot_{i+1}) */
#define GK_KID_STENCIL 1 /* Poisson-5 stencil sweeps incl. fused preconditioner sweeps */
#define GK_KID_SCALE 2   /* normalisation V(:,j+1) = w / h */
#define GK_KID_UPDATE 3  /* x += V y */
#define GK_KID_COMM 4    /* all-reduce / broadcast (RCCL, local group or device exchange) */
#define GK_KID_OTHER 5
#define GK_KID_RES 6     /* resident MGS-R step: whole cascade + norm + scale in one launch */
#define GK_KID_PREC 7    /* temporal-blocked Chebyshev(k) passes (k_cheb_fused); GK_PREC_MG: one whole V-cycle */
#define GK_KID_HALO 8    /* halo lines with the slab neighbours (RCCL send/recv, local group or device exchange) */
#define GK_KID_GRAPH 9   /* one launch-path MGS-R step replayed as a hipGraph (its 2j projections, all-reduces, scale) */
/* short-recurrence passes (gk_sr_*): GK_KID_SR + the pass kind of gk_sr.hpp --
 * 0 cg_p, 1 cg_x, 2 cg_z, 3 bi_p, 4 bi_pc, 5 bi_s, 6 bi_sc, 7 st1, 8 st2 (line
 * marches), 9 bi_x, 10 bi_pe, 11 bi_se, 12 dot (element-wise), 13 cg_xz, 14 bi_pz,
 * 15 bi_sz (two-level marches: cbpr2 and the operator in one pass) */
#define GK_KID_SR 10
#define GK_NKID 26

typedef struct gk_ctx gk_ctx;
typedef struct gk_group gk_group;

const char *gk_last_error(void);
int gk_version(void);
/* Which runtime this library is running on (bench.py / smoke() report it):
 * hipRuntimeGetVersion, hipDriverGetVersion, ncclGetVersion, and the files the
 * process mapped for libamdhip64 and librccl (dladdr of one of their symbols),
 * NUL-terminated into hip_path / rccl_path (capacity `len` bytes each). */
int gk_runtime_info(int *hip_runtime, int *hip_driver, int *rccl, char *hip_path, char *rccl_path, int len);

/* ------------------------------------------------------------ context ---- */
/* Create a context on HIP device `device` for an N x N grid, owning lines
 * [line0, line0+nlines), Krylov dimension m (restart length).  Allocates
 * V (n x (m+1)), the work vectors and the reduction slabs in HBM. */
int gk_create(int device, int nside, int line0, int nlines, int m, gk_ctx **out);
int gk_destroy(gk_ctx *ctx);
/* Multi-GPU: rank 0 calls gk_comm_unique_id, the 128 bytes are shared out of
 * band, then every rank calls gk_comm_init.  Ranks own consecutive slabs
 * (rank r-1 below rank r).  `max_lines` = the largest nlines of any rank. */
int gk_comm_unique_id(unsigned char id[128]);
int gk_comm_init(gk_ctx *ctx, int nranks, int rank, int max_lines, const unsigned char id[128]);
/* In-process communicator with the same message pattern as RCCL: nranks
 * contexts of ONE process (any devices, e.g. all on one GPU for testing the
 * slab decomposition), each driven by its own host thread. */
int gk_group_create(int nranks, gk_group **out);
int gk_group_destroy(gk_group *g);
int gk_comm_init_local(gk_ctx *ctx, gk_group *g, int rank, int max_lines);
/* Device exchange ("xgmi" back-end, SURVEY 8e "custom xGMI flag-based
 * all-reduce"): the per-projection all-reduces, the Householder broadcast and
 * the halo lines are moved by the GPUs themselves -- each rank stores tagged
 * 8-byte granules straight into every peer's receive region over xGMI, and
 * the consumer polls its own region -- instead of one RCCL call per
 * reduction.  Same results on every rank (rank-order sums).
 *   gk_comm_init_xgmi   decomposition without RCCL (ranks on distinct GPUs,
 *                       or several processes on one GPU);
 *   gk_xchg_handle      this rank's IPC handle (64 bytes) to share out of band;
 *   gk_xchg_open        map every rank's region (handles: nranks x 64 bytes,
 *                       rank order) and route collectives through it;
 *   gk_xchg_local       the same for a gk_group (in-process, after every
 *                       member's gk_comm_init_local); GK_ERR_STATE at once
 *                       when the members on this device, plus one stream
 *                       (the null stream), exceed the process's hardware
 *                       queues (GPU_MAX_HW_QUEUES, HIP's default 4): streams
 *                       would share a queue, and a spinning exchange kernel
 *                       could sit in front of its peer's kernel until the
 *                       deadline;
 *   gk_xchg_enable      0: back to RCCL / the local group, 1: device exchange;
 *   gk_xchg_selftest    collective check of the reduction and halo paths with
 *                       a deadline; GK_ERR_COMM if any granule is missing or
 *                       wrong.  Also usable after gk_comm_init (RCCL present):
 *                       a failed test leaves the exchange disabled.  (Tests:
 *                       env GK_DEBUG_SELFTEST_FAIL=<rank> makes that rank fail
 *                       at once without taking part; its peers then miss
 *                       their deadline.)
 * Usable together with gk_comm_init (then RCCL remains the fallback).
 * A missed deadline during a solve (GK_ERR_COMM, naming the late rank or
 * workgroup) retires the exchange of that context: its later exchanges fail at
 * once and gk_xchg_enable(1) refuses.  It does NOT switch back to RCCL by
 * itself -- the caller does, on EVERY rank together, with gk_xchg_enable(0)
 * (switching only the rank that saw the miss would desynchronise the ranks). */
int gk_comm_init_xgmi(gk_ctx *ctx, int nranks, int rank, int max_lines);
int gk_xchg_handle(gk_ctx *ctx, unsigned char handle[64]);
int gk_xchg_open(gk_ctx *ctx, const unsigned char *handles);
int gk_xchg_local(gk_ctx *ctx);
int gk_xchg_enable(gk_ctx *ctx, int on);
int gk_xchg_selftest(gk_ctx *ctx, int timeout_ms);
int gk_local_size(gk_ctx *ctx, long long *nloc);
/* What this context's collectives actually run on: kind = GK_COMM_NONE (single
 * rank), GK_COMM_RCCL, GK_COMM_LOCAL (gk_group) or GK_COMM_XGMI (device
 * exchange on); nranks_seen = the communicator's own rank count (ncclCommCount
 * for RCCL, the mapped exchange regions for the device exchange). */
#define GK_COMM_NONE 0
#define GK_COMM_RCCL 1
#define GK_COMM_LOCAL 2
#define GK_COMM_XGMI 3
int gk_comm_info(gk_ctx *ctx, int *kind, int *nranks_seen);
/* First contact between two devices of the node (no context needed): whether
 * `device` can map `peer`'s memory (hipDeviceCanAccessPeer) and the link type
 * and hop count between them (hipExtGetLinkTypeAndHopCount; link_type as HIP's
 * HSA_AMD_LINK_INFO_TYPE: 4 = xGMI, 2 = PCIe).  bench.py logs it for every rank
 * pair of an N-GPU line.  device == peer: can_access 1, hops 0. */
int gk_peer_info(int device, int peer, int *can_access, int *link_type, int *hops);
/* Collective, every rank together: the mean cost (us, HIP events on the
 * context stream) of one all-reduce of a projection's partial slab and of one
 * halo exchange (one grid line with each neighbour) through the collective in
 * use (device exchange, RCCL or the local group), over `iters` back-to-back
 * calls.  Diagnostic (bench.py reports it beside a multi-GPU line); leaves
 * the reduction slots and halo buffers overwritten. */
int gk_comm_latency(gk_ctx *ctx, int iters, double *allreduce_us, double *halo_us);

/* Preconditioner: kind GK_PREC_*, params (cbpr2: params[0..1] as
 * chebyshev.f90:19-25; CHEB: interval ends params[0..1]), degree (CHEB and MG).
 *
 * GK_PREC_MG: a V-cycle of aggregation multigrid on 2 x 2 blocks for the 5-point operator.
 * With piecewise-constant prolongation P and the 4-member sum P^T, P^T A_N P = 2 A_{N/2}:
 * every level runs the same unscaled stencil on a smaller square grid (the geometric
 * choice -- twice the Galerkin correction, the classical over-correction of unsmoothed
 * aggregates).  Levels: N_0 = N; while N_l is even and N_l / 2 >= 8, N_{l+1} = N_l / 2.
 * On every level but the last, with Cheb = Chebyshev(degree) on params[0..1] from zero:
 *   z = Cheb(r); rc = P^T (r - A z); z += P MG_{l+1}(rc); out = z + Cheb(r - A z).
 * The last level is Chebyshev(nu_c) on its exact spectrum interval, nu_c the smallest
 * degree in 1..64 whose error bound 1 / cosh((nu + 1) acosh sigma) is <= 0.1 (capped at
 * 64: grids with few factors of two, e.g. 514 -> 257, get a weak coarse solve and more
 * iterations).  Symmetric positive definite: it serves PCG as well as GMRES / BiCGSTAB,
 * on either side.  The hierarchy is built here and freed by gk_destroy or the next
 * gk_set_precond.  GK_ERR_ARG: odd N or N / 2 < 8, a degree outside 1..8, an empty
 * interval.  GK_ERR_STATE: a context that is not the whole grid on one rank (any
 * communicator, line0 != 0, nlines != N); gk_comm_init* on an MG context return the same.
 * The stateless gk_precond_apply has no multigrid (GK_ERR_ARG). */
int gk_set_precond(gk_ctx *ctx, int kind, const double *params, int nparams, int degree);
/* The multigrid hierarchy.  info (GK_MG_INFO_LEN ints): [0] the number of levels L + 1,
 * [1] the last level's sweep count nu_c, [2] the smoother degree (gk_mg_info; 0 from the
 * plan query), [3 .. 3 + L] the level sides N_0 .. N_L, zeros after.
 * gk_mg_plan_query: pure host, for a grid of side nside; no device is touched.
 * gk_mg_info: the live hierarchy of a context whose preconditioner is GK_PREC_MG
 * (GK_ERR_STATE otherwise).
 * gk_mg_transfer: diagnostic / test hook on host arrays between level `level` and the
 * next (f = N_level^2, c = N_{level+1}^2 doubles) of an MG context --
 *   what 0  out(c) = P^T a(f)                  the plain restriction
 *   what 1  out(c) = P^T (a(f) - A b(f))       the fused residual-restriction march
 *   what 2  out(f) = a(f) + P b(c)             the prolongation
 * It overwrites the hierarchy's work vectors and ends an open cycle, as gk_apply does. */
#define GK_MG_INFO_LEN 35
int gk_mg_plan_query(int nside, int *info);
int gk_mg_info(gk_ctx *ctx, int *info);
int gk_mg_transfer(gk_ctx *ctx, int what, int level, const double *a, const double *b, double *out);
/* Side of the preconditioner in the MGS-R cycle (context state; default left; kept
 * across gk_set_precond).
 *   GK_SIDE_LEFT   the reference: w = M^-1 A V(:,j), and the host's stopping quantity
 *                  |g(j+1)| / ||b|| is the PRECONDITIONED residual ||M^-1 (b - A x)||
 *                  over the unpreconditioned ||b|| (gmres_mgsr.f90:307,383).
 *   GK_SIDE_RIGHT  w = A M^-1 V(:,j), x += M^-1 (V y): the Arnoldi residual is the
 *                  true residual b - A x, so |g(j+1)| / ||b|| is what gk_true_residual
 *                  returns, to rounding.  gk_mgs_cycle_start takes w = b - A x
 *                  without the preconditioner; the cascade, norm and scale of a step
 *                  are unchanged (resident launch, hipGraph and launch path all
 *                  apply); gk_update_x forms t = V y, applies M^-1 and adds.  With
 *                  the identity preconditioner both sides run the same launches
 *                  (bit-identical).  A M^-1 v runs as ONE launch for cbpr2 on one
 *                  rank (GK_TUNE_RIGHT_FUSED), else as the preconditioner's own
 *                  launches followed by the stencil.
 * Setting the side ends a running gk_sr_* solve and an open GMRES cycle (steps
 * return GK_ERR_STATE until the next cycle start).  The side is the MGS-R cycle's.
 * The Householder cycle takes its side per call: GK_HH_PREC_RIGHT preconditions on
 * the right whatever the context's side is, and GK_HH_PREC_LEFT, like the
 * short-recurrence solvers, on the left only -- with side right and a preconditioner
 * other than the identity, gk_hh_cycle_start / gk_hh_step_async with
 * precondition = GK_HH_PREC_LEFT and gk_sr_start return GK_ERR_STATE. */
#define GK_SIDE_LEFT 0
#define GK_SIDE_RIGHT 1
int gk_set_precond_side(gk_ctx *ctx, int side);
/* The operator's shift (context state; default 0): A := A_poisson + sigma I, sigma >= 0 --
 * implicit diffusion steps (I + tau (-Laplace)), screened Poisson, pseudo-time continuation,
 * after scaling.  One rule everywhere: with s = ((W + E) + N) + S in the stencil's order,
 *   y = fma(diag, c, -s),  diag = fl(4 + sigma),
 * ONE fused multiply-add on every path (stencil sweeps, cbpr2 marches, the Chebyshev passes,
 * the short-recurrence marches, the multigrid residuals); at sigma = 0 it is bit-identical to
 * 4 c - s.  A stays symmetric positive definite, so every solver and preconditioner applies.
 *   cbpr2 / Chebyshev: params are the caller's interval as before, now that of A + sigma I
 *     (e.g. (8.2 + sigma, 0.2 + sigma)); nothing is added for the caller.
 *   GK_PREC_MG: level l runs the same stencil with sigma_l = 4^l sigma (the shift
 *     rediscretised as the operator is; Galerkin's 4 sigma, not its half), diag_l =
 *     fl(4 + sigma_l).  params are level 0's interval; level l smooths on it moved by
 *     sigma_l - sigma; the last level on its exact interval plus sigma_L, with nu_c recomputed
 *     from that interval (gk_mg_info reports it).  Setting the shift refreshes a live hierarchy
 *     in place (no allocation); gk_set_precond(MG) after it builds by the same rule.
 * Setting the shift ends a running gk_sr_* solve and an open GMRES cycle (as
 * gk_set_precond_side does) and, when the value changes, drops the captured step graphs,
 * which hold diag by value.  b and x are not touched: gk_set_rhs_ones after gk_set_shift
 * gives b = (A + sigma I) 1.  No device allocation, no synchronisation of its own.  On N
 * ranks every rank sets the same value (not checked, like params); halos and collectives
 * are unaffected.  GK_ERR_ARG: sigma < 0, not finite, or > 1e12 (4^l sigma stays finite).
 * gk_poisson5, gk_precond_apply and gk_mg_plan_query keep meaning sigma = 0. */
int gk_set_shift(gk_ctx *ctx, double sigma);
int gk_get_shift(gk_ctx *ctx, double *sigma);
/* Storage precision of the Krylov basis in the MGS-R cycle (context state; default
 * GK_BASIS_F64; beyond the reference).
 *   GK_BASIS_F64  every column an FP64 vector (the reference).
 *   GK_BASIS_F32  the compressed basis (CB-GMRES): a column is STORED as FP32 -- the new
 *                 column is float(w_i / h), the division in FP64, one round-to-nearest-
 *                 even conversion, 0 when h = 0 -- and widened exactly wherever it is
 *                 read.  w, every dot, every AXPY, the Hessenberg column, the Givens
 *                 rotations and x stay FP64, in the expressions and order of the FP64
 *                 step, so the Arnoldi relation holds for the stored vectors and a
 *                 restart, which recomputes the true residual in FP64, converges to
 *                 FP64 accuracy.  A projection of the resident step (k_mgs_wcb) moves 8 B
 *                 per unknown instead of 16.  Within one cycle the basis resolves a
 *                 residual reduction of about 2^-24 only: the host drivers close a cycle
 *                 once final_err(j) < 2^-20 g(1) / ||b|| without declaring convergence
 *                 (the next cycle starts from the FP64 true residual).
 *                 No allocation: FP32 column k lives at float offset k * ld of the basis
 *                 allocation (its lower half); the operator stage reads two FP64 vectors
 *                 from the free upper half, column 1 and the newest column widened, so no
 *                 operator or preconditioner kernel changes (both sides apply).  Needs
 *                 m >= 3 (GK_ERR_ARG) and a single-rank context: GK_ERR_STATE on a context
 *                 with a communicator, and gk_comm_init* on an F32 context returns
 *                 GK_ERR_STATE.  MGS-R only: gk_hh_cycle_start / gk_hh_step_async return
 *                 GK_ERR_STATE.  GK_TUNE_RES_BLOCK > 1 and GK_TUNE_RES_PF are ignored
 *                 (the strict projection order runs); the step runs as one resident
 *                 launch (gk_res_info: GK_RES_CB) or, with GK_TUNE_RES 0, m + 1 > 500, or
 *                 several contexts sharing the device without GK_TUNE_RES 1, launch by
 *                 launch (hipGraph replays as with FP64 columns).  gk_update_x,
 *                 gk_get_basis (the exact stored values, widened) and gk_mgs_verr (the
 *                 tree-reduced Gram) read the float columns.  gk_sr_* and gk_vec_* are
 *                 unaffected: they own their columns as FP64 and start from their own data.
 * Setting the precision ends a running gk_sr_* solve and an open GMRES cycle (steps
 * return GK_ERR_STATE until the next gk_mgs_cycle_start) and drops the captured step
 * graphs.  Setting GK_BASIS_F64 again gives back the default solve bit for bit.
 * gk_cb_plan_query: pure host computation of the resident F32 step's plan for a slab of
 * nloc unknowns on cus / share compute units with Krylov dimension m;
 * info[GK_CB_INFO_LEN]: workgroups G, RW, LW (register / LDS chunks of 256 double2 of w
 * per thread the kernel is built for), r2e, l2e (those a workgroup uses), dynamic LDS
 * bytes, resident double2, streamed double2, whether the resident launch applies, and
 * the kernel's static LDS bytes. */
#define GK_BASIS_F64 0
#define GK_BASIS_F32 1
#define GK_CB_INFO_LEN 10
int gk_set_basis_precision(gk_ctx *ctx, int prec);
int gk_get_basis_precision(gk_ctx *ctx, int *prec);
int gk_cb_plan_query(long long nloc, int cus, int share, int m, long long *info);
/* Orthogonalisation scheme of the MGS-R cycle's Arnoldi step (context state; default
 * GK_ORTH_MGSR; kept across gk_set_precond, gk_set_precond_side and gk_set_tuning).
 *   GK_ORTH_MGSR  modified Gram-Schmidt with one reorthogonalisation, the reference
 *                 (gmres_mgsr.f90:341-360): 2j dependent dots per step.
 *   GK_ORTH_CGS2  classical Gram-Schmidt with one full reorthogonalisation (beyond the
 *                 reference; it changes the operation order, so it is opt-in).  After the
 *                 unchanged operator stage, step j runs two sweeps of
 *                     s_k = <w, V_k>, k = 1..j, every dot on the SAME w (N ranks: rank totals)
 *                     w_e = ((w_e - s_1 V_1,e) - s_2 V_2,e) .. - s_j V_j,e   (k ascending)
 *                     H(k,j) = s_k (sweep 1)  /  H(k,j) + s_k (sweep 2)
 *                 then h = ||w||, V(:,j+1) = w / h as in the MGS-R step (h = 0 writes zeros).
 *                 Three reductions per step whatever j is: 7 launches (batched dots, their
 *                 fixed-order reduce, the j-column AXPY; twice; the scale) and 3 all-reduces
 *                 against the launch path's 2j + 1 of each.  No in-launch waiting, so it runs
 *                 on every communicator and for every m.  The MGS step of a CGS2 context
 *                 never runs a resident launch: gk_res_info(hh = 0) reports GK_RES_NONE, and
 *                 GK_TUNE_RES, GK_TUNE_RES_BLOCK and GK_TUNE_RES_PF are ignored for it (they
 *                 keep their values for when GK_ORTH_MGSR comes back).  GK_TUNE_GRAPH,
 *                 GK_TUNE_PROJ_NT and GK_TUNE_PROJ_BLOCKS apply.  A dots workgroup batches 8
 *                 columns against each load of w; GK_CGS_KB=16 in the environment of
 *                 gk_create builds the context on batches of 16 (an A/B knob: any other
 *                 value is GK_ERR_ARG).  The Householder cycle, gk_sr_* and
 *                 gk_vec_* are unaffected.  FP64 columns only: GK_ORTH_CGS2 on a
 *                 GK_BASIS_F32 context and gk_set_basis_precision(GK_BASIS_F32) on a
 *                 GK_ORTH_CGS2 context return GK_ERR_STATE (a float-column instantiation
 *                 of the three kernels is the natural follow-up).
 * Any other value returns GK_ERR_ARG.  Setting the scheme ends a running gk_sr_* solve and
 * an open GMRES cycle (steps return GK_ERR_STATE until the next gk_mgs_cycle_start) and
 * drops the captured step graphs, as gk_set_basis_precision does.  Setting GK_ORTH_MGSR
 * again gives back the default solve bit for bit. */
#define GK_ORTH_MGSR 0   /* the reference: gmres_mgsr.f90:341-360 (default) */
#define GK_ORTH_CGS2 1   /* beyond the reference */
int gk_set_orthogonalization(gk_ctx *ctx, int scheme);
int gk_get_orthogonalization(gk_ctx *ctx, int *scheme);
/* Right-hand side b (local part, host) or b = A*1 built on device
 * (the manufactured RHS of every reference driver, test_poisson_mf.f90:39-40).
 * A is the shifted operator: for b = (A + sigma I) 1 call gk_set_shift first. */
int gk_set_rhs(gk_ctx *ctx, const double *b_local);
int gk_set_rhs_ones(gk_ctx *ctx);
/* beta0 = ||b||_2 (global). */
int gk_rhs_norm(gk_ctx *ctx, double *beta0);
/* x = 0 (x0 is always 0 in the reference, gmres_mgsr.f90:304). */
int gk_zero_x(gk_ctx *ctx);
int gk_get_x(gk_ctx *ctx, double *x_local);
/* Copy column col (0-based) of a device basis to the host (nloc doubles):
 * which = 0: V(:,col+1) -- the MGS-R Krylov basis, or the Householder
 * reflectors P(:,col+1) (gmres_hh.f90 keeps P in the same array);
 * which = 1: the Householder basis rebuilt by gk_hh_verr (calculate_verr's V).
 * Diagnostic only (the orthogonality tests evaluate the reference's formula on
 * the device basis). */
int gk_get_basis(gk_ctx *ctx, int which, int col, double *out);
/* The inverse of gk_get_basis(which = 0): overwrite column col (0-based, 0..m) of the
 * MGS-R Krylov basis / the Householder reflectors with in[0..nloc).  Diagnostic / test
 * support only (the single-step tests plant known columns in an open cycle).
 * FP64 basis: the nloc doubles are copied as they are.
 * FP32 basis: every value must be finite and exactly representable as a float, otherwise
 * GK_ERR_ARG and nothing is written (no silent second rounding).  The values are stored
 * as floats; the same values widened become the operator's input (vjw), and the first
 * dot's partner (v1w) when col = 0 -- the state a cycle leaves that produced this column
 * last.  The column set LAST is therefore the next step's operator input: plant column
 * j - 1 last before gk_mgs_step(j).
 * Ends a running gk_sr_* solve (its vectors share the allocation), as gk_set_x does; does
 * not close an open GMRES cycle and does not touch the captured step graphs (they hold
 * pointers only). */
int gk_set_basis(gk_ctx *ctx, int col, const double *in);
int gk_set_x(gk_ctx *ctx, const double *x_local);
/* Host-array operator application on this context's slab (clobbers the
 * work vectors; not between cycle start and update):  what = 0: out = A in
 * (stencil_vector, poisson.f90:33-77); what = 1: out = M^-1 in (precond).
 * A is A_poisson + sigma I (gk_set_shift), here and in gk_true_residual. */
int gk_apply(gk_ctx *ctx, int what, const double *in, double *out);
/* ||b - A x|| / ||b|| (global, true unpreconditioned residual). */
int gk_true_residual(gk_ctx *ctx, double *rel);

/* -------------------------------------------- MGS-R cycle (gmres_mgsr.f90) */
/* w = M^-1 (b - A x); beta = ||w||; V(:,1) = w / beta   (:314-329).
 * Returns beta (= g(1)). */
int gk_mgs_cycle_start(gk_ctx *ctx, double *beta);
/* Arnoldi step j (1 <= j <= m): z = A V(:,j); w = M^-1 z; two MGS passes
 * over V(:,1:j) accumulating H(1:j,j); h = ||w||; V(:,j+1) = w / h
 * (:336-363, :384).  hcol[0..j] = H(1:j+1, j) before any Givens rotation. */
int gk_mgs_step(gk_ctx *ctx, int j, double *hcol);
/* The same step split in two so the host can run the Givens rotation of
 * step j while the GPU already works on step j+1: gk_mgs_step_async enqueues
 * step j and returns; gk_mgs_step_wait(j) blocks until its Hessenberg column
 * is available.  Enqueueing step j+1 before step j's convergence test is
 * harmless: a step only writes w and V(:,j+1) and its own column slot. */
int gk_mgs_step_async(gk_ctx *ctx, int j);
int gk_mgs_step_wait(gk_ctx *ctx, int j, double *hcol);
/* x += V(:,1:n_out) y  (:400-406). */
int gk_update_x(gk_ctx *ctx, const double *y, int n_out);
/* Orthogonality diagnostic v_err(1:n_out+1) (:414-420) from the Gram matrix
 * of V(:,1:n_out+1) computed on device.  zero_last != 0 treats V(:,n_out+1)
 * as the zero column gmres_mgsr_mf leaves after an in-cycle exit (:172-176). */
int gk_mgs_verr(gk_ctx *ctx, int n_out, int zero_last, double *v_err);

/* -------------------------------------- Householder cycle (gmres_hh.f90) */
/* The `precondition` argument of gk_hh_cycle_start, gk_hh_step and gk_hh_step_async
 * (any other value: GK_ERR_ARG):
 *   GK_HH_PREC_NONE   gmres_hh_omp: the operator alone.
 *   GK_HH_PREC_LEFT   gmres_hh_prec_omp: w = M^-1 A v_j, and |g(j+1)| / ||b|| is the
 *                     PRECONDITIONED residual over ||b||.  GK_ERR_STATE on a context whose
 *                     side is right (gk_set_precond_side) with a preconditioner other than
 *                     the identity.
 *   GK_HH_PREC_RIGHT  beyond the reference, whatever the context's side is: the cycle
 *                     starts from w = b - A x, step j forms w = A M^-1 v_j -- ONE launch
 *                     for cbpr2 on one rank (k_right_cbpr2, GK_TUNE_RIGHT_FUSED), else the
 *                     preconditioner's launches and the stencil -- and gk_hh_update_x adds
 *                     M^-1 (P_1..P_n [y;0]), so |g(j+1)| / ||b|| is what gk_true_residual
 *                     returns, to rounding: the quantity side right gives the MGS-R cycle.
 *                     The reflection chains, the fused close (GK_TUNE_HH_FUSE),
 *                     GK_TUNE_RES_FOLD and GK_TUNE_HH_NORM_ORDER apply unchanged.  With
 *                     the identity preconditioner it runs the launches of GK_HH_PREC_NONE
 *                     (bit-identical).
 * A cycle is right-preconditioned or not from its start on: a step whose `precondition`
 * is GK_HH_PREC_RIGHT in a cycle started otherwise, or the reverse, returns GK_ERR_STATE. */
#define GK_HH_PREC_NONE 0
#define GK_HH_PREC_LEFT 1
#define GK_HH_PREC_RIGHT 2
/* Cycle start.  GK_HH_PREC_NONE / _RIGHT: w = b - A x (gmres_hh_omp :243-253);
 * _LEFT: w = M^-1 (b - A x) (gmres_hh_prec_omp :425-436).  Builds reflector
 * P(:,1); returns g1 = g(1) = -sign(beta, w(1)). */
int gk_hh_cycle_start(gk_ctx *ctx, int precondition, double *g1);
/* Step j: v = P_1..P_j e_j; w = A v (_LEFT: M^-1 A v; _RIGHT: A M^-1 v); w = P_j..P_1 w;
 * hcol[0..j] = H(1:j+1,j) (H(j+1,j) = -sign(||w(j+1:n)||, w(j+1)));
 * builds P(:,j+1)  (:255-321 / :438-502). */
int gk_hh_step(gk_ctx *ctx, int j, int precondition, double *hcol);
/* Split form of gk_hh_step (see gk_mgs_step_async). */
int gk_hh_step_async(gk_ctx *ctx, int j, int precondition);
int gk_hh_step_wait(gk_ctx *ctx, int j, double *hcol);
/* x += P_1..P_n_out [y;0]  (:350-378); after a cycle started with GK_HH_PREC_RIGHT:
 * t = P_1..P_n_out [y;0], x += M^-1 t -- for cbpr2 on one rank the cbpr2 sweep with an
 * accumulating output (t and x read, x written: one launch, GK_TUNE_RIGHT_FUSED), else
 * the preconditioner's launches into a work vector and the add; bit-identical x. */
int gk_hh_update_x(gk_ctx *ctx, const double *y, int n_out);
/* calculate_verr (:568-593): v_err(i) = sum_{j<i} 2 (V_i.V_j)^2, V rebuilt
 * from the reflectors on device (extra n x n_out buffer). */
int gk_hh_verr(gk_ctx *ctx, int n_out, double *v_err);

/* ------------------------------------------------ spectrum estimate ---- */
/* k Lanczos steps on A from a deterministic pseudo-random start vector (the
 * same for any slab decomposition); returns the extreme Ritz values of the
 * k x k tridiagonal (Sturm bisection on the host).  The README-promised
 * eigenvalue estimate for the Chebyshev parameters (README.md:11; the
 * reference hard-codes params, chebyshev.f90:20).  Clobbers work vectors.
 * A is A_poisson + sigma I (gk_set_shift): the bounds are those at sigma = 0
 * plus sigma (the same Krylov space). */
int gk_lanczos_bounds(gk_ctx *ctx, int k, double *lmin, double *lmax);

/* ------------------------------------------- device vector primitives ---- */
/* For the short-recurrence solvers that share the operator / preconditioner
 * seam (pcg_omp src/cg.f90:154-234, pbicgstab_omp src/bicgstab.f90:91-182):
 * context-resident vectors by id: GK_VEC_X = x, GK_VEC_B = b, 2 .. m+2 =
 * scratch (the Krylov columns).  Scalars come back to the host, as the
 * reference computes them in `single` blocks. */
#define GK_VEC_X 0
#define GK_VEC_B 1
#define GK_LC_COPY 0   /* out = a                  */
#define GK_LC_AXPY 1   /* out = a + s1*b           */
#define GK_LC_AXPY2 2  /* out = (a + s1*b) + s2*c  */
#define GK_LC_XPAYMZ 3 /* out = a + s1*(b - s2*c)  */
#define GK_LC_ZERO 4   /* out = 0                  */
int gk_vec_count(gk_ctx *ctx, int *count);
/* what = 0: out = A in; what = 1: out = M^-1 in; what = 2: out = A M^-1 in, the
 * operator of a right-preconditioned step by the step's own route (whatever the
 * context's side is); in != out.  A is A_poisson + sigma I (gk_set_shift). */
int gk_vec_apply(gk_ctx *ctx, int what, int in, int out);
/* result = <a, b> over all ranks (synchronous). */
int gk_vec_dot(gk_ctx *ctx, int a, int b, double *result);
int gk_vec_lincomb(gk_ctx *ctx, int form, int out, int a, int b, int c, double s1, double s2);

/* ------------------------------------- fused short-recurrence solvers ---- */
/* pcg_omp (src/cg.f90:154-234) and pbicgstab_omp (src/bicgstab.f90:91-182)
 * with every scalar on the device: one iteration is 2 (PCG) or 3 (BiCGSTAB)
 * fused passes (gmres_amd/csrc/gk_sr.hpp; with cbpr2 on one rank the
 * preconditioner runs inside two-level marches; N ranks or
 * GK_TUNE_SR_TWO_LEVEL 0: 3 / 5 passes), no host round trip per dot.  They replace the call sequence the reference's solvers make
 * through the operator / preconditioner seam (interfaces.f90:13-27): the
 * Fortran drivers pcg_drive / bicgstab_drive queue iterations in chunks and
 * read one status per chunk.  Vectors: the context's Krylov columns 0..7
 * and its w / vj work vectors (needs m >= 7); x stays in HBM (gk_get_x).
 *
 * gk_sr_start: x = 0, r = b; PCG: z = M^-1 r, p = z (cg.f90:174-187);
 *   BiCGSTAB: r0 = p = r (bicgstab.f90:112-118).  max_iter bounds the total
 *   number of iterations gk_sr_iterate may queue (the history's length).
 * gk_sr_iterate: queue k more iterations, no host wait.  Iterations after the
 *   first with res < tol return at entry on the device (`if (converged) cycle`).
 * gk_sr_status: wait = 0: for the oldest queued chunk; 1: for everything
 *   queued.  *executed = iterations run, *done = the first iteration with
 *   res < tol (0: none), *res = residual of the last executed iteration.
 * gk_sr_history: hist[0..n) = res after iterations 1..n (n <= *executed).
 * gk_set_precond / gk_set_rhs(_ones) / gk_set_x / gk_mgs_cycle_start /
 * gk_hh_cycle_start end a running solve (they change its data or reuse its
 * vectors): gk_sr_iterate / status / history then return GK_ERR_STATE until
 * the next gk_sr_start. */
#define GK_SR_PCG 0
#define GK_SR_BICGSTAB 1
int gk_sr_start(gk_ctx *ctx, int solver, double tol, int max_iter);
int gk_sr_iterate(gk_ctx *ctx, int k);
int gk_sr_status(gk_ctx *ctx, int wait, int *executed, int *done, double *res);
int gk_sr_history(gk_ctx *ctx, double *hist, int n);

/* ---------------------------------------------------------- profiling ---- */
/* enable = 1: every launch is bracketed by HIP events on the context stream;
 * enable = S > 1: only the launches of MGS-R steps with j % S == 0 (launch
 * durations do not depend on j, so the per-launch average is unbiased while
 * the event overhead drops S-fold).  gk_profile_read returns the summed
 * device time (ms) and launch count per kernel id since the last reset. */
int gk_profile_enable(gk_ctx *ctx, int enable);
int gk_profile_reset(gk_ctx *ctx);
int gk_profile_read(gk_ctx *ctx, int kid, double *total_ms, long long *launches);
/* Time split of the resident launches, measured inside them (wall clock of
 * thread 0 of every workgroup): mode 1 enables and zeroes, 2 zeroes, 0
 * disables, -1 only reads.  For the launches of kind `which` (0 MGS-R step,
 * 1 Householder UP chain, 2 Householder DOWN chain) since the last reset:
 * the mean over workgroups of the time streaming passes, the time waiting in
 * the in-launch all-gathers, and the launch total, summed over launches (out
 * pointers may be NULL to skip reading). */
int gk_profile_res_split(gk_ctx *ctx, int mode, int which, double *pass_ms, double *wait_ms, double *total_ms,
                         long long *launches);
/* The same split per workgroup (blockIdx order, summed over launches): the
 * arrival skew of the in-launch all-gathers shows as the spread of pass_ms. */
int gk_profile_res_wg(gk_ctx *ctx, int which, double *pass_ms, double *wait_ms, int maxwg, int *nwg);
/* All-gather trace of one resident launch: for every workgroup and in-launch exchange, the
 * wall-clock ticks at which its partial was published and at which it held the grid total
 * (tools/res_trace.py: arrival skew vs propagation).  arm 1: trace the MGS-R step launches
 * of Arnoldi step j from now on (mode must be 0; each overwrites the last); 0: off; -1: read
 * the last traced launch into out[nwg][nx][2]. */
int gk_profile_res_trace(gk_ctx *ctx, int arm, int j, int mode, unsigned long long *out, int maxwg, int maxx,
                         int *nwg, int *nx, double *tick_per_ms);
int gk_sync(gk_ctx *ctx);

/* ------------------------------------------- resident-step variant plan ---- */
/* Which resident kernel an Arnoldi step (and a Householder chain) runs on.
 * Selection is by the slab's local length and the workgroups available
 * (compute units / contexts sharing the device), so a 2- / 4- / 8-GPU split
 * of one grid selects a different variant than the single-GPU run does:
 *   GK_RES_NONE       no resident launch (one launch per projection);
 *   GK_RES_PREFETCH   k_mgs_res<R2 in 2,4,8, PF, control wave>: small slabs;
 *   GK_RES_PAIRS      k_mgs_res<12, 0>: w and the running column in registers;
 *   GK_RES_PAIRS_LDS  k_mgs_res<12, 18>: the same plus w of 18 chunks per
 *                     workgroup in LDS, the rest streamed;
 *   GK_RES_WONLY      k_mgs_wres: w only, in registers + LDS (large slabs);
 *   GK_RES_WCOL       k_mgs_wpc: w in registers and the running Krylov column cached
 *                     (registers + LDS) -- 8 B per unknown per projection for slabs of
 *                     up to 64 x 256 double2 per workgroup (one GPU of 4096^2 / 2 and
 *                     of 8192^2 / 8), in 512-thread workgroups (two waves per SIMD); slabs
 *                     of <= 16 chunks per thread (4096^2 / 4) keep the whole column in
 *                     registers (r2 = 16, l2 = 0);
 *   GK_RES_BLOCKED    k_mgs_blk (gmres_amd/csrc/gk_blk.hpp): the blocked-projection MGS-R
 *                     step of GK_TUNE_RES_BLOCK > 1 -- one all-gather per block of S
 *                     projections; r2 / l2 = cached column chunks per block slot in
 *                     registers / LDS, blk = S;
 *   GK_RES_CB         k_mgs_wcb (gmres_amd/csrc/gk_cb.hpp): the step of a GK_BASIS_F32
 *                     context on float columns -- w only, in registers + LDS, chunks of
 *                     256 double2; r2 / l2 = the chunks the kernel is built for
 *                     (gk_res_info only: gk_cb_plan_query is its planner).
 * info[GK_RES_INFO_LEN]: variant, workgroups G, R2, L2, prefetch, control
 * wave, w-only, non-temporal column loads, register / LDS chunks per
 * workgroup in use, dynamic LDS bytes, resident double2 of the slab, and
 * whether the w-only MGS step runs its software-pipelined pass (GK_TUNE_RES_PIPE; 1 / 0),
 * (gk_res_info only) whether the Arnoldi step's Chebyshev(k) pass forms z = A v in its own
 * stage 0 (1 / 0; -1 on a multi-rank context whose smallest slab is not known
 * until its first solve), the threads per workgroup (= double2 per chunk), the
 * projection block S (1: strict MGS-R), and `carry`: the chunks of the pipelined pass's ring
 * that the launches load across each all-gather (GK_TUNE_RES_PIPE_CARRY; 0: none).
 * gk_res_plan_query: pure host computation for a slab of nloc unknowns on a
 * device with `cus` compute units shared by `share` contexts; hh != 0 the
 * reflection chains' plan; nt: -1 auto (from nloc), 0 / 1 forced; block: the
 * GK_TUNE_RES_BLOCK value (1, 2 or 4) of the MGS step's plan.  No device
 * is touched (the CPU tests pin every production split with it).
 * gk_res_info: the plan this context uses now (its tuning, communicator and
 * sharing applied); variant GK_RES_NONE when steps run launch by launch. */
#define GK_RES_NONE 0
#define GK_RES_PREFETCH 1
#define GK_RES_PAIRS 2
#define GK_RES_PAIRS_LDS 3
#define GK_RES_WONLY 4
#define GK_RES_WCOL 5
#define GK_RES_BLOCKED 6
#define GK_RES_CB 7
#define GK_RES_INFO_LEN 17
int gk_res_plan_query(long long nloc, int cus, int share, int hh, int nt, int block, long long *info);
int gk_res_info(gk_ctx *ctx, int hh, long long *info);

/* Launch-policy knobs (defaults are the tuned values; for A/B measurement).
 *   GK_TUNE_PROJ_NT        1: non-temporal loads of the Krylov columns in the
 *                          projection kernel (keeps w resident in the 256 MB
 *                          Infinity Cache); 0: plain loads; -1: auto (default:
 *                          non-temporal when a vector exceeds 48 MiB)
 *   GK_TUNE_PROJ_BLOCKS    workgroups of the projection kernel (0 = auto)
 *   GK_TUNE_STENCIL_BLOCKS target workgroups of the stencil sweeps (0 = auto)
 *   (retired keys, unknown now and never reused: 3, 17 and 26 -- the reversed projection
 *   walk, the w-only step's stencil prologue and the look-ahead blocked step -- were
 *   measured slower and removed in round 5, DESIGN.md 3.1 / 3.1c / 3.4 keep the numbers;
 *   4, 5 and 12 -- the projection kernel's contiguous-range mapping, its forced unroll
 *   (the auto rule stays: 4 loads in flight for one trip per thread or fewer, else 2) and
 *   the switch that streamed what the pairs variant holds in LDS -- recorded no win and
 *   nothing set them)
 *   GK_TUNE_CHEB_FUSED     1 (default): Chebyshev(k <= 8) as temporal-blocked passes of up to
 *                          4 sweeps each (single slab, even N); 0: one launch per sweep
 *   GK_TUNE_XCHG_TIMEOUT_MS deadline of one device-exchange wait (default 20000)
 *   GK_TUNE_RES            resident MGS-R step (one persistent launch per Arnoldi step, w and the
 *                          running Krylov column held in registers, dots all-gathered inside the
 *                          launch): -1 auto (default: on for a single rank or the device exchange,
 *                          m <= 512, one context per device), 1 also with several contexts on one
 *                          device (their streams must then run concurrently), 0 off (one launch
 *                          per projection)
 *   GK_TUNE_RES_R2         cap of register-resident double2 per thread and array: 0 auto, 2/4/8/12
 *   GK_TUNE_RES_SHARE      contexts sharing this device (resident launches use CUs / share
 *                          workgroups; gk_comm_init_local sets it to the group size)
 *   GK_TUNE_RES_TIMEOUT_MS deadline of one in-launch wait (default 20000); a miss fails the step
 *                          with GK_ERR_COMM and switches the context to the launch path
 *   GK_TUNE_RES_WONLY      large slabs: -1 (default) pick by the modelled bytes per projection,
 *                          1 always, 0 never the w-only variant (one wave per SIMD, ~490 registers
 *                          per lane: w in registers + LDS, both columns streamed)
 *   GK_TUNE_RES_PIPE       the w-only MGS step's software-pipelined pass (the column loads of the
 *                          next half-batch in flight while one is consumed; bit-identical
 *                          results): -1 (default) the build's choice (GK_RES_PIPE), 1 on, 0 off.
 *                          It runs only where every workgroup holds its full 89 + 39 chunks and
 *                          nothing is streamed (4096^2 on 256 CUs); gk_res_info reports whether
 *                          the launches run it (`pipe`)
 *   GK_TUNE_RES_PIPE_CARRY the pipelined pass with the head of its ring carried across the
 *                          all-gather: the first GK_RES_PIPE_CARRY chunk pairs of the next pass are
 *                          loaded while the workgroup waits for the dot (the ring registers are
 *                          otherwise empty there), and the L2 touches start that many chunks
 *                          later; bit-identical results.  -1 (default) the build's choice
 *                          (GK_RES_PIPE_CARRY chunks; 0 = not built), 0 off, anything else on.
 *                          Only where the pipelined pass runs and only on a single rank (on N
 *                          ranks the pushers drain their loads before they publish, so carried
 *                          loads would sit on every rank's critical path: those launches keep the
 *                          plain pipelined pass); gk_res_info reports the chunks carried (`carry`)
 *   GK_TUNE_VERR_ORDER     1 (default): the v_err diagnostics (gk_mgs_verr, gk_hh_verr) use the
 *                          reference's dot_product order, one running sum per dot (bit-identical
 *                          to the reference's formula on the same basis; single rank); 0: tree
 *                          reduction (fast; N ranks always use it)
 *   GK_TUNE_HH_FUSE        1 (default): with the w-only resident variant a Householder step folds
 *                          its small launches into the reflection chains -- the DOWN chain builds
 *                          e_j itself, the UP chain ends with the reflector fix-up and
 *                          P(:,j+1) = w/||w|| (gmres_hh.f90:306-318); 0: separate k_set_unit,
 *                          k_hh_fix and k_scale launches
 *   GK_TUNE_CHEB_STEN      1 (default): the Arnoldi step's Chebyshev(k <= 8) pass forms z = A v
 *                          itself in a stage ahead of its levels (no stencil launch, no z vector;
 *                          N >= 128, slabs of at least k + 1 lines); 0: stencil launch + pass
 *   GK_TUNE_GRAPH          1 (default): a launch-path MGS-R step (RCCL ranks, device-exchange ranks
 *                          with the resident step off, or one rank with it off) is captured once
 *                          per step index j as a hipGraph -- its 2j projection launches, 2j + 1
 *                          all-reduces (ncclAllReduce / k_xchg captured as graph nodes; a replayed
 *                          k_xchg takes its sequence number from a device base set before each
 *                          replay) and the normalisation -- and replayed in later cycles;
 *                          0: launched call by call.  A capture that fails switches it off for
 *                          the context (gk_last_error keeps the reason).
 *   GK_TUNE_RES_QDEF       k_mgs_res with non-temporal columns (pairs / pairs+lds): 1 = the LDS-held
 *                          and streamed parts read each pass's dot column V_q with the default
 *                          policy, so the next pass's AXPY column (the same V_q) is an
 *                          Infinity-Cache hit (the w-only kernel's policy); 0 = both
 *                          non-temporal; -1 (default) = the measured choice
 *   GK_TUNE_RES_FOLD       1 (default): N ranks on the device exchange -- the MGS step's first dot
 *                          <w, V(:,1)> (Householder: <w, P_1>) is summed across ranks inside the
 *                          resident launch (its rank-total hop) instead of by a k_xchg launch
 *                          before it; 0: the launch
 *   GK_TUNE_RES_PC         column-cache variant (GK_RES_WCOL): -1 (default) where its modelled
 *                          bytes per projection are fewer than both the pairs and the w-only
 *                          variants'; 0 never; 1 wherever the slab fits
 *   GK_TUNE_RES_BLOCK      1 (default): the strict MGS-R step (gmres_mgsr.f90:341-360), one
 *                          in-launch all-gather per projection; 2 or 4 (opt-in): the blocked
 *                          step k_mgs_blk -- the projections of each sweep in blocks of S
 *                          columns, ONE all-gather per block carrying its S dots and the Gram
 *                          terms of its newest column, the h formed by MGS's exact-arithmetic
 *                          recurrence h_k = <w,V_k> - sum_{l<k} h_l <V_l,V_k> (the two sweeps
 *                          stay separate, so the reorthogonalisation still sees w after the
 *                          whole first sweep): 2 (1 + ceil((j-1)/S)) all-gathers per step
 *                          instead of 2j.  Not bit-identical to the strict step (within the
 *                          residual-history tolerance of DESIGN.md 4.3).  MGS-R resident
 *                          steps only; Householder and the launch path stay strict.
 *   GK_TUNE_RES_PF         the STRICT MGS-R step on the blocked kernel with blocks of 1
 *                          (k_mgs_blk<S = 1>: the reference's projection order, one all-gather
 *                          per projection) whose next dot column is prefetched into LDS during
 *                          each all-gather; gk_res_info reports variant blocked, blk 1.  0
 *                          (default): the strict kernels; 1: for every slab up to 32 chunks of
 *                          512 double2 per workgroup (faster on one GPU at 16 chunks only;
 *                          DESIGN.md 3.1c)
 *   GK_TUNE_WATCHDOG_MS    limit of every host wait on the context's stream (gk_sync, the step
 *                          waits, gk_update_x ...); 0 (default) = twice the longest device
 *                          deadline plus a minute.  Past it the wait returns GK_ERR_COMM (a
 *                          kernel of the context was never scheduled) and the context is
 *                          BROKEN: every later call returns GK_ERR_STATE; gk_destroy frees it
 *                          once its stream drains (bounded by the same limit; else it is kept)
 *   GK_TUNE_HH_NORM_ORDER  0 (default): the Householder reflector norms (gmres_hh.f90:251-253,
 *                          307, 315) tree-reduced in the resident chains; 1 (one rank): taken
 *                          in the reference's own order -- flang-rt's NORM2, a running max and
 *                          scaled sum over the vector (k_norm2_seq) -- so the device basis
 *                          carries the reference's normalisation rounding (the v_err band of
 *                          DESIGN.md 4.3 becomes two-sided); the step runs unfused.  A
 *                          diagnostic mode: one sequential pass per norm (~0.1 ms per 16 K)
 *   GK_TUNE_SR_BLOCKS      target workgroups of the short-recurrence line marches (gk_sr_*; 0 =
 *                          auto, 512: each marches JT = lines x windows / 512 grid lines, up to
 *                          256 -- long marches re-read fewer neighbour lines)
 *   GK_TUNE_SR_TWO_LEVEL   1 (default): with the cbpr2 preconditioner on one rank the
 *                          short-recurrence solvers run the preconditioner and the operator
 *                          next to it in one two-level march (PCG 2 passes per iteration,
 *                          BiCGSTAB 3); 0: one pass each (3 / 5).  Bit-identical results;
 *                          read by gk_sr_start
 *   GK_TUNE_RIGHT_FUSED    1 (default): side right with cbpr2 on one rank forms w = A M^-1 v in
 *                          one two-level line march (k_right_cbpr2: v and the dot partner
 *                          read, w written, z = M^-1 v never stored); 0: the route of N ranks
 *                          and of Chebyshev(k) -- the preconditioner's launch, then the
 *                          stencil.  Bit-identical w.  The same key selects the update of a
 *                          GK_HH_PREC_RIGHT cycle (gk_hh_update_x): 1 the cbpr2 sweep with the
 *                          accumulating output, x += M^-1 t in one launch; 0 the sweep into a
 *                          work vector, then the add.  Bit-identical x
 *   GK_TUNE_SPIN_WAIT      1 (default): gk_mgs_step_wait / gk_hh_step_wait spin on the step's
 *                          event; 0: hipEventSynchronize (may sleep in the driver per step)
 *   GK_TUNE_MG_FUSED       1 (default): the multigrid cycle forms each level's restricted
 *                          residual P^T (r - A z) in one line march (z and r read, a quarter
 *                          vector written, the residual never stored); 0: the residual
 *                          stencil into a work vector, then the plain restriction.
 *                          Bit-identical results */
#define GK_TUNE_PROJ_NT 0
#define GK_TUNE_PROJ_BLOCKS 1
#define GK_TUNE_STENCIL_BLOCKS 2
#define GK_TUNE_CHEB_FUSED 6
#define GK_TUNE_XCHG_TIMEOUT_MS 7
#define GK_TUNE_RES 8
#define GK_TUNE_RES_R2 9
#define GK_TUNE_RES_SHARE 10
#define GK_TUNE_RES_TIMEOUT_MS 11
#define GK_TUNE_RES_WONLY 13
#define GK_TUNE_VERR_ORDER 14
#define GK_TUNE_HH_FUSE 15
#define GK_TUNE_CHEB_STEN 16
#define GK_TUNE_SPIN_WAIT 18
#define GK_TUNE_GRAPH 19
#define GK_TUNE_RES_QDEF 20
#define GK_TUNE_RES_PC 21
#define GK_TUNE_RES_FOLD 22
#define GK_TUNE_RES_BLOCK 23
#define GK_TUNE_WATCHDOG_MS 24
#define GK_TUNE_HH_NORM_ORDER 25
#define GK_TUNE_RES_PF 27
#define GK_TUNE_SR_BLOCKS 28
#define GK_TUNE_SR_TWO_LEVEL 29
#define GK_TUNE_RES_PIPE 30
#define GK_TUNE_RIGHT_FUSED 31
#define GK_TUNE_RES_PIPE_CARRY 32
#define GK_TUNE_MG_FUSED 33 /* GK_PREC_MG contexts only */
int gk_set_tuning(gk_ctx *ctx, int key, int value);
/* Test hook: hold = 1 enqueues on the context's stream a wait for a mapped host
 * word that only hold = 0 writes (hipStreamWaitValue32) -- every later kernel of
 * the context then stays unscheduled until the release, as with a hardware queue
 * that is never mapped; it exercises the host watchdog (GK_TUNE_WATCHDOG_MS). */
int gk_debug_hold_stream(gk_ctx *ctx, int hold);

/* ------------------------- stateless kernel API (caller device memory) ---- */
/* y = A x on lines [0,nlines) of an N-wide slab; halo_lo / halo_hi are the
 * grid lines just below / above the slab (NULL at the physical boundary)
 * -- stencil_vector, src/problems/poisson.f90:33-77.  stream: hipStream_t. */
int gk_poisson5(int nside, int nlines, const double *x, const double *halo_lo,
                const double *halo_hi, double *y, void *stream);
/* ... and y = (A + sigma I) x by gk_set_shift's rule, y = fma(fl(4 + sigma), c, -s);
 * GK_ERR_ARG for sigma < 0, not finite or > 1e12.  gk_poisson5 is sigma = 0. */
int gk_poisson5_shift(int nside, int nlines, double sigma, const double *x, const double *halo_lo,
                      const double *halo_hi, double *y, void *stream);
/* z = M^-1 r for the single-slab case (precond, src/interfaces.f90:20-27);
 * scratch: 3 vectors of N*N doubles. */
int gk_precond_apply(int nside, int kind, const double *params, int degree, const double *r,
                     double *z, double *scratch, void *stream);
/* Fused MGS projection (gmres_mgsr.f90:343-358): h = <w,va>;
 * w -= h*va; result[0] = h (device). */
int gk_mgs_project(long long n, double *w, const double *va, double *result, void *stream);
/* result[0] = <a,b> (device). */
int gk_dot(long long n, const double *a, const double *b, double *result, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GMRES_HIP_H */
