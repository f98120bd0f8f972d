"""The aggregation multigrid V-cycle preconditioner (GK_PREC_MG) on the GPU against its
restatement on host arrays (tests/mg_data.py: the CPU oracle's stencil and Chebyshev sweeps
per level, numpy sums in the stated order).

Every element-wise stage is a single IEEE operation on both sides (no contraction), so
transfers and whole cycles are compared with np.array_equal; the fused reductions differ
in summation order only and take the tolerances the Chebyshev epilogue tests use.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import mg_data

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TUNE_CHEB_FUSED = 6
TUNE_MG_FUSED = 33


def _data(n, N, seed):
    """Random values on a ramp that is symmetric in nothing: a transposed or shifted index
    cannot cancel."""
    i, j = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64))  # [j, i]
    ramp = (0.37 * i + 1.13 * j + 0.011 * i * j).reshape(-1) / N
    assert n == N * N
    return np.random.default_rng(seed).standard_normal(n) + ramp


@functools.lru_cache(maxsize=None)
def _ref_cycle(N, params, degree, seed):
    from oracle import oracle as orc

    v = _data(N * N, N, seed)
    out = mg_data.mg(orc, v, N, params, degree)
    v.setflags(write=False)
    out.setflags(write=False)
    return v, out


@functools.lru_cache(maxsize=None)
def _ref_pcg(N):
    from oracle import oracle as orc

    return mg_data.pcg(orc, N)[0]


def _ctx_col(c, k):
    """V(:,k+1) of a context, through the device vector API (copy to x)."""
    from gmres_amd import _native as nat

    nat.check(nat.hip().gk_vec_lincomb(c.handle, 0, 0, 2 + k, 0, 0, 0.0, 0.0), "gk_vec_lincomb")
    return c.get_x()


# ------------------------------------------------------------------ transfers ---
@pytest.mark.parametrize("N,level", [(16, 0), (20, 0), (130, 0), (514, 0), (48, 0), (48, 1),
                                     (128, 0), (128, 3), (256, 2), (256, 4), (1450, 0), (1456, 0), (1456, 1)])
def test_transfers_bitexact(oracle, N, level):
    """gk_mg_transfer what 0 / 1 / 2 against numpy.  16: lanes masked; 20: a coarse grid of
    10; 130: a wave seam at fine column 128 and several line tiles; 514: two points in a
    second workgroup along i, coarse 257 odd; 48: also level 1 -> 2 (24 -> 12); 128 and 256:
    the last transfer of five and six levels (16 -> 8) and one in the middle (64 -> 32).

    The steady state of the kernels, with 256 threads per workgroup.  The restriction marches
    JT = even-ceil(N ceil(N / 512) / 2048) lines per workgroup, clamped to [2, 64]: 2 for every
    N <= 1364, where the residual-restriction's rolling lines m / c / p / n never carry from one
    line pair to the next.  1450: ceil(1450 / 512) = 3 workgroups along i, 1450 * 3 / 2048 =
    2.12 -> 3 -> JT = 4, and 1450 = 362 * 4 + 2 leaves a clipped last tile of one pair; the
    prolongation wants ceil(725^2 / 256) = 2054 workgroups and gets 2048, so its grid-stride
    loop runs a second time in the first six.  1456: 1456 * 3 / 2048 = 2.13 -> JT = 4 in 364
    whole tiles, and ceil(728^2 / 256) = 2071 > 2048; its level 1 (728 -> 364) is back at JT = 2
    on two workgroups along i, with 518 workgroups of prolongation."""
    import gmres_amd as ga

    with ga.Context(N, 4) as c:
        c.set_precond("mg")
        sides = c.mg_info()["sides"]
        assert sides == mg_data.levels(N)
        nf, ncs = sides[level], sides[level + 1]
        for seed in (1, 2):
            a = _data(nf * nf, nf, 100 * N + seed)
            b = _data(nf * nf, nf, 200 * N + seed)
            ec = _data(ncs * ncs, ncs, 300 * N + seed)
            assert np.array_equal(c.mg_transfer(0, level, a), mg_data.restrict(a, nf))
            assert np.array_equal(c.mg_transfer(1, level, a, b), mg_data.resid_restrict(oracle, a, b, nf))
            assert np.array_equal(c.mg_transfer(2, level, a, ec), mg_data.prolong_add(a, ec, nf))


# -------------------------------------------------------------------- V-cycle ---
@pytest.mark.parametrize("N", [16, 48, 100, 130, 514, 128, 256, 1450, 1456])
def test_vcycle_bitexact(oracle, N):
    """c.apply(v, 1) against the restatement: degrees 1..3, two intervals, and the four
    routes GK_TUNE_MG_FUSED x GK_TUNE_CHEB_FUSED -- one result.  gk_vec_apply(1) and (2)
    likewise, the latter composed with the oracle's stencil.

    128 and 256: five and six levels (128, 64, 32, 16, 8 and 256, ...), three and four
    intermediate levels whose eight vectors come out of one allocation.  1450 (sides 1450, 725)
    and 1456 (1456, 728, 364, 182, 91), on the default interval and degree only: the shapes
    of test_transfers_bitexact inside a cycle -- restriction tiles of four lines, clipped
    (1450) and whole (1456), a second grid-stride pass of the prolongation on level 0 (on
    level 1 of 1456 it has 518 workgroups), a second pass of the closing add (its 2048
    workgroups cover 2048 * 256 double2 = 1024^2 elements of 1450^2), and on 725 the coarse
    Chebyshev degree at its cap of 64."""
    import gmres_amd as ga

    sweep = [(p, d) for p in ((8.0, 1.0), (8.2, 2.0)) for d in (1, 2, 3)]
    if N > 1024:
        sweep = [(mg_data.DEFAULT_PARAMS, mg_data.DEFAULT_DEGREE)]
    if N == 1450:
        assert mg_data.coarse(725)[2] == 64
    with ga.Context(N, 4) as c:
        for params, degree in sweep:
            v, ref = _ref_cycle(N, params, degree, N + degree)
            for mgf in (1, 0):
                for chf in (1, 0):
                    c.tune(TUNE_MG_FUSED, mgf)
                    c.tune(TUNE_CHEB_FUSED, chf)
                    c.set_precond("mg", params, degree)
                    got = c.apply(v, 1)
                    assert np.array_equal(got, ref), (params, degree, mgf, chf, float(np.abs(got - ref).max()))
        c.tune(TUNE_MG_FUSED, 1)
        c.tune(TUNE_CHEB_FUSED, 1)
        c.set_precond("mg")
        v, ref = _ref_cycle(N, mg_data.DEFAULT_PARAMS, mg_data.DEFAULT_DEGREE, N + mg_data.DEFAULT_DEGREE)
        c.set_x(v)
        c.vec_apply(1, 0, 2)  # x -> V(:,1)
        assert np.array_equal(_ctx_col(c, 0), ref)
        c.set_x(v)
        c.vec_apply(2, 0, 2)  # A M^-1 x, the right-preconditioned step's operator
        assert np.array_equal(_ctx_col(c, 0), oracle.stvec(ref, N))


# ------------------------------------------------------------------ epilogues ---
@pytest.mark.parametrize("N", [48, 130])
def test_left_epilogues(oracle, N):
    """MG on the left: the cycle start's beta = ||M^-1 b|| (ACC_NORM on the closing add) and
    step 1's H(1,1) (ACC_DOT) against the restatement, to the tolerances of
    test_fused_chebyshev_norm_epilogue / _dot_epilogue_step; V(:,1) bit for bit."""
    import gmres_amd as ga

    b = oracle.rhs_ones(N)
    w = mg_data.mg(oracle, b, N)
    bref = float(np.sqrt(np.sum(w * w)))
    with ga.Context(N, 10) as c:
        c.set_precond("mg")
        c.set_rhs_ones()
        beta = c.mgs_cycle_start()
        v1 = _ctx_col(c, 0)
        assert beta == pytest.approx(bref, rel=1e-14)
        assert np.array_equal(v1, w / beta)
        c.zero_x()  # _ctx_col overwrote x
        assert c.mgs_cycle_start() == beta
        h = c.mgs_step(1)
    w1 = mg_data.mg(oracle, oracle.stvec(v1, N), N)
    h1 = float(w1 @ v1)
    h1 = h1 + float((w1 - h1 * v1) @ v1)  # MGS-R: the reorthogonalisation's correction
    print(f"N={N} beta {beta!r} ref {bref!r}  h11 {h[0]!r} ref {h1!r}")
    assert np.allclose(h[0], h1, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("N", [130, 1450])
def test_left_epilogues_general_rhs(oracle, N):
    """test_left_epilogues from a right-hand side without the square's symmetries
    (general_data.general_rhs through set_rhs), where a partial read from the wrong end or a
    dropped tail changes the sum: beta = ||M^-1 b|| from ACC_NORM on the closing add against the
    long-double norm of the restated M^-1 b, and V(:,1) = w / beta bit for bit.  At 1450 the
    closing add's 2048 workgroups make a second and a third grid-stride pass (1450^2 / 2 double2
    over 2048 * 256 threads: 2.005).

    The bound is 64 eps relative: a sum of squares has condition 1, so a summation tree of
    depth d is off by at most d eps (first order) plus the rounding of the products and of the
    root.  The device's tree: at most 6 sequential additions per thread (two per pass), 6
    levels across a wave and 3 additions across the waves, then the slab of at most 2048
    partials in 8 sequential additions per thread, 6 levels and 3 additions -- depth 32.  Two
    float64 trees of the host on this data land at 1.4 and 7.7 eps."""
    import gmres_amd as ga
    from tests.general_data import EPS, MARGIN
    from tests.test_gpu_general_rhs import _gen

    _, b = _gen(oracle, N)
    w = mg_data.mg(oracle, b, N)
    wl = w.astype(np.longdouble)
    bref = float(np.sqrt(np.sum(wl * wl)))
    with ga.Context(N, 4) as c:
        c.set_precond("mg")
        c.set_rhs(b)
        beta = c.mgs_cycle_start()
        v1 = _ctx_col(c, 0)
    dev = abs(beta - bref) / bref
    print(f"N={N}: beta {beta!r} long double {bref!r}: dev {dev / EPS:.2f} eps, dev/bound {dev / (MARGIN * EPS):.3e}")
    assert dev <= MARGIN * EPS
    assert np.array_equal(v1, w / beta)


def test_left_step_1450(oracle):
    """One left-preconditioned MGS-R step on planted columns at 1450^2, m = 2, j = 1 and 2, on
    the launch path (test_gpu_step_known_answer.py::test_preconditioned_step, whose bounds
    these are; pinned on the CPU by test_general_data.py): the first dot comes from
    k_mg_add<ACC_DOT> in its second and third grid-stride pass, where the partner column's
    index has to follow the sum's."""
    from tests import test_gpu_step_known_answer as ka
    from tests.general_data import MG_DEGREE, MG_PARAMS

    N, m = 1450, 2
    c = ka._open(N, m, [(ka.T_RES, 0)], side="left", prec=("mg", MG_DEGREE), params=MG_PARAMS)
    with c:
        assert c.res_info()["variant"] is None
        ka._check(oracle, c, N, m, [1, 2], "left-mg-1450 launch", op=("left", "mg", MG_DEGREE, MG_PARAMS))


# ------------------------------------- solves from a general right-hand side ---
# b = A x_true without the square's symmetries (tests/test_gpu_general_rhs.py), every solver
# family held to the restatement with the restated cycle as M^-1.  MG gains a decade per
# iteration, so m = 4 and tol 1e-12 give a history of three cycles.
G_N, G_M, G_TOL, G_CAP = 130, 4, 1e-12, 6
_host: dict = {}


def _host_mgsr(oracle, side):
    """(the MGS-R restatement at one thread, |hist_res(1 thread) - hist_res(7 threads)|)."""
    from tests.right_gmres_host import gmres_mgsr_host
    from tests.test_gpu_general_rhs import _gen

    key = ("mgsr", side)
    if key not in _host:
        b = _gen(oracle, G_N)[1]
        h1, h7 = (gmres_mgsr_host(oracle, G_N, G_M, prec="mg", degree=mg_data.DEFAULT_DEGREE, side=side, tol=G_TOL,
                                  params=mg_data.DEFAULT_PARAMS, max_cycles=G_CAP, b=b, threads=th) for th in (1, 7))
        assert h1.n_cycles == h7.n_cycles and 2 <= h1.n_cycles < G_CAP
        _host[key] = (h1, np.abs(h1.hist_res - h7.hist_res))
    return _host[key]


def _mg_solve(oracle, side, tunes=(), orth=None, basis=None, method="mgsr", tol=G_TOL):
    """One device solve of the 130^2 case from set_rhs(b): (result, gk_true_residual, plan, profile)."""
    import gmres_amd as ga
    from tests.test_gpu_general_rhs import _gen

    with ga.Context(G_N, G_M) as c:
        for k, v in tunes:
            c.tune(k, v)
        c.set_precond("mg", side=side)
        if basis is not None:
            c.set_basis(basis)
        if orth is not None:
            c.set_orth(orth)
        c.set_rhs(_gen(oracle, G_N)[1])
        plan = c.res_info(hh=method == "hh")
        c.profile(True)
        c.profile_reset()
        if method == "mgsr":
            r = ga.gmres_mgsr(c, tol, variant=ga.MGSR_MF, max_cycles=G_CAP, want_hist=True)
        else:
            r = ga.gmres_hh(c, tol, precondition=side, max_cycles=G_CAP, want_hist=True)
        prof = c.profile_read()
        c.profile(False)
        return r, c.true_residual(), plan, prof


def _n_outs(r):
    return [int(np.count_nonzero(row)) for row in r.hist_ferr]


@pytest.mark.parametrize("route", ["launch", "resident"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_mgsr_general_rhs(oracle, side, route):
    """MGS-R to 1e-12 against tests/right_gmres_host.py with prec = "mg": the same cycles, the
    same n_out in every cycle, hist_res within 1e-5 r + 1e-13 (test_gpu_general_rhs.py::
    test_right_side_general_rhs) and never less than 10 x the restatement's own 1-vs-7-thread
    spread, x within 1e-9 max |x_true| of the restatement's.  The launch path, and the resident
    prefetch step on the forcing of test_gpu_general_rhs.py's MGSR_ROUTES at this N."""
    from tests import test_gpu_general_rhs as gr

    x_true, _ = gr._gen(oracle, G_N)
    h, spread = _host_mgsr(oracle, side)
    tunes = [(gr.T_RES, 0)] if route == "launch" else gr._res_tunes(2, 8, -1, -1)
    r, true, plan, prof = _mg_solve(oracle, side, tunes)
    what = f"mg mgsr {side} {route}"
    print(f"{what}: plan {plan}; cycles {r.n_cycles} (host {h.n_cycles}), n_outs {_n_outs(r)} (host {h.n_outs})")
    if route == "launch":
        assert plan["variant"] is None and prof["res"][1] == 0, (plan, prof)
    else:
        assert plan["variant"] == "prefetch" and prof["res"][1] > 0, (plan, prof)
    assert r.n_cycles == h.n_cycles and _n_outs(r) == h.n_outs and r.n_out == h.n_out
    gr._hist(r.hist_res, h.hist_res, 1e-5 * h.hist_res + 1e-13, spread, what + " vs host")
    gr._solution(r, true, h.x, x_true, what)


@pytest.mark.parametrize("side", ["left", "right"])
def test_cgs2_general_rhs(oracle, side):
    """CGS2 against the same MGS-R restatement by the rule tests/test_gpu_cgs2.py holds CGS2 to
    MGS-R histories with (_contract: 1e-5 r + 1e-13 per cycle), the same cycle count, and x
    within 1e-9 max |x_true| of the restatement's."""
    from tests import test_gpu_general_rhs as gr

    x_true, _ = gr._gen(oracle, G_N)
    h, spread = _host_mgsr(oracle, side)
    r, true, plan, _ = _mg_solve(oracle, side, orth="cgs2")
    what = f"mg cgs2 {side}"
    print(f"{what}: cycles {r.n_cycles} (host {h.n_cycles}), n_outs {_n_outs(r)} (host {h.n_outs})")
    assert plan["variant"] is None and r.n_cycles == h.n_cycles
    gr._hist(r.hist_res, h.hist_res, 1e-5 * h.hist_res + 1e-13, spread, what + " vs host MGS-R")
    gr._solution(r, true, h.x, x_true, what)


@pytest.mark.parametrize("route", ["launch", "resident"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_fp32_basis_general_rhs(oracle, side, route):
    """The FP32 basis to 1e-8 against tests/cb_gmres_host.py with prec = "mg" by the rule of
    test_gpu_general_rhs.py::test_fp32_basis_general_rhs: the same cycle count, n_out within
    one, hist_res within max(1e-6, 100 S_c) relative, S_c the restatement's 1-vs-8-thread
    spread; x within 1e-5 max |x_true| of x_true once converged (of the restatement's x, 1e-6,
    if not)."""
    from gmres_amd import _native as nat
    from tests import test_gpu_general_rhs as gr
    from tests.cb_gmres_host import gmres_cb_host

    x_true, b = gr._gen(oracle, G_N)
    tol = 1e-8
    key = ("cb", side)
    if key not in _host:
        _host[key] = tuple(gmres_cb_host(oracle, G_N, G_M, prec="mg", degree=mg_data.DEFAULT_DEGREE, side=side, tol=tol,
                                         params=mg_data.DEFAULT_PARAMS, max_cycles=G_CAP, threads=th, b=b) for th in (1, 8))
    h, h8 = _host[key]
    k8 = min(h.n_cycles, h8.n_cycles)
    S = np.maximum.accumulate(np.abs(h8.hist_res[:k8] - h.hist_res[:k8]) / h.hist_res[:k8])
    r, true, plan, _ = _mg_solve(oracle, side, [] if route == "resident" else [(gr.T_RES, 0)], basis="f32", tol=tol)
    what = f"mg fp32 basis {side} {route}"
    print(f"{what}: plan {plan}; cycles {r.n_cycles} (host {h.n_cycles}), n_out {r.n_out} (host {h.n_out})")
    assert plan["variant"] == (nat.RES_VARIANTS[nat.GK_RES_CB] if route == "resident" else None), plan
    assert r.n_cycles == h.n_cycles and abs(r.n_out - h.n_out) <= 1
    k = min(len(S), r.n_cycles)
    rel = np.abs(r.hist_res[:k] - h.hist_res[:k]) / h.hist_res[:k]
    bound = np.maximum(1e-6, 100.0 * S[:k])
    print(f"{what}: worst dev/bound of hist_res {np.max(rel / bound):.3e}; restatement 1-vs-8-thread spread {S.max():.3e}")
    assert k == r.n_cycles and np.all(rel <= bound)
    converged = h.final_err[h.n_out - 1] < tol
    err = np.max(np.abs(r.x - (x_true if converged else h.x))) / np.max(np.abs(x_true))
    print(f"{what}: converged {converged}, max |x - {'x_true' if converged else 'x_host'}| / max |x_true| {err:.3e}")
    assert err < (1e-5 if converged else 1e-6)
    assert abs(true - r.hist_res[-1]) <= 1e-12 * r.hist_res[-1]


@pytest.mark.parametrize("side", ["left", "right"])
def test_householder_general_rhs(oracle, side):
    """Householder GMRES(m) to 1e-12 (the CPU oracle has no multigrid): as many cycles as the
    MGS-R restatement, both being GMRES(m) in exact arithmetic; x within 1e-9 max |x_true| of
    x_true, which no permuted x meets on this data; gk_true_residual is the last history entry."""
    from tests import test_gpu_general_rhs as gr

    x_true, _ = gr._gen(oracle, G_N)
    h, _ = _host_mgsr(oracle, side)
    r, true, _, _ = _mg_solve(oracle, side, method="hh")
    what = f"mg hh {side}"
    print(f"{what}: cycles {r.n_cycles} (MGS-R restatement {h.n_cycles}); residuals {r.hist_res.tolist()} "
          f"(restatement {h.hist_res.tolist()})")
    assert r.n_cycles == h.n_cycles
    gr._solution(r, true, x_true, x_true, what)


SR_ITERS = 12
SR_CASES = [(s, N) for s in ("pcg", "pbicgstab") for N in (48, 130)]


def _host_sr(oracle, solver, N):
    """The restated PCG / BiCGSTAB history of SR_ITERS iterations and x at 1 and at 7 threads."""
    from tests.test_gpu_general_rhs import _gen

    key = (solver, N)
    if key not in _host:
        b = _gen(oracle, N)[1]
        out = []
        for th in (1, 7):
            oracle.set_threads(th)
            try:
                if solver == "pcg":
                    out.append(mg_data.pcg(oracle, N, tol=0.0, max_iter=SR_ITERS, b=b, full=True)[2:])
                else:
                    out.append(mg_data.pbicgstab(oracle, b, N, SR_ITERS))
            finally:
                oracle.set_threads(1)
        _host[key] = out
    return _host[key]


@pytest.mark.parametrize("solver,N", SR_CASES)
def test_short_recurrence_general_rhs(oracle, solver, N):
    """A fixed 12 iterations of the fused PCG / BiCGSTAB passes (tol 0) against
    mg_data.pcg / mg_data.pbicgstab with the same b.  The restated histories fall a decade
    (PCG) and two (BiCGSTAB) per iteration, and their 1-vs-7-thread spread stays near 1e-13
    relative: every iteration carries signal.

    PCG: every entry within 1e-9 relative (the level test_gpu_general_rhs.py::
    test_short_recurrence_general_rhs holds the fused passes to above 1e-4 of the first entry;
    here over all 12, the device differing from the restatement in summation order only, as
    its two thread counts do), never less than 10 x that spread; x within 1e-9 max |x_true| of
    the restatement's and 1e-6 of x_true.  BiCGSTAB: the first decade to 1e-9 (_close_early)
    and the whole history inside tests/sr_band.py's band, 100 x the running spread; x likewise."""
    import gmres_amd as ga
    from tests.sr_band import bicgstab_band
    from tests.test_gpu_general_rhs import _gen
    from tests.test_gpu_sr import _close_early

    x_true, b = _gen(oracle, N)
    (h1, x1), (h7, _) = _host_sr(oracle, solver, N)
    assert len(h1) == len(h7) == SR_ITERS
    with ga.Context(N, 8) as c:
        c.set_precond("mg")
        c.set_rhs(b)
        s = ga.SrSolve(c, solver, 0.0, SR_ITERS)
        s.iterate(SR_ITERS)
        ex, done, res = s.status()
        assert (ex, done) == (SR_ITERS, 0)
        h = s.history(ex)
        x = c.get_x()
    assert h[-1] == res
    spread = np.abs(h7 - h1) / h1
    dev = np.abs(h - h1) / h1
    what = f"mg {solver} N={N}"
    if solver == "pcg":
        lim = np.maximum(1e-9, 10.0 * spread)
        print(f"{what}: history {h.tolist()}; worst dev/bound {np.max(dev / lim):.3e}; restatement 1-vs-7-thread spread "
              f"{spread.max():.3e}")
        assert np.all(dev <= lim), (dev, lim)
    else:
        early = _close_early(h, h1, 1e-9)
        ok, worst = bicgstab_band(h, h1, h7)
        print(f"{what}: history {h.tolist()}; first decade {early:.3e} (bound 1e-9); worst |ln ratio| / band {worst:.3e}; "
              f"restatement 1-vs-7-thread spread {spread.max():.3e}, device max rel dev {dev.max():.3e}")
        assert early <= 1e-9
        assert ok, worst
    scale = np.max(np.abs(x_true))
    e_host, e_true = np.max(np.abs(x - x1)) / scale, np.max(np.abs(x - x_true)) / scale
    print(f"{what}: max |x - x_host| / max |x_true| {e_host:.3e} (bound 1e-9), max |x - x_true| / max |x_true| {e_true:.3e}")
    assert e_host <= 1e-9 and e_true <= 1e-6


@pytest.mark.parametrize("solver", ["pcg", "pbicgstab"])
def test_chunking_is_bit_identical(oracle, solver):
    """test_gpu_sr.py::test_chunking_is_bit_identical with the V-cycle inside every iteration,
    from a general b at 48^2: 40 iterations queued as 40 x 1 (eager launches), 1 x 40 (two
    captured 16-iteration graphs + 8 eager) and 3 + 37 -- bit-identical histories and x.  The
    solves reach rounding level after about 15 iterations and go on: the recurrences' scalars
    stay finite and non-zero on this data (the restated residuals fall to 1e-40 and 1e-76
    without a zero denominator), so all 40 iterations run."""
    import gmres_amd as ga
    from tests.test_gpu_general_rhs import _gen

    N, K = 48, 40
    b = _gen(oracle, N)[1]
    outs = []
    for chunks in ([1] * K, [K], [3, K - 3]):
        with ga.Context(N, 8) as c:
            c.set_precond("mg")
            c.set_rhs(b)
            s = ga.SrSolve(c, solver, 0.0, K)
            for k in chunks:
                s.iterate(k)
            ex, done, res = s.status()
            assert (ex, done) == (K, 0)
            h = s.history(ex)
            assert h[-1] == res and np.all(np.isfinite(h)) and np.all(h > 0.0)
            outs.append((h, c.get_x()))
    print(f"mg {solver} chunking: history[0], [15], [39] = {outs[0][0][0]!r}, {outs[0][0][15]!r}, {outs[0][0][39]!r}")
    for h, x in outs[1:]:
        assert np.array_equal(h, outs[0][0])
        assert np.array_equal(x, outs[0][1])


# --------------------------------------------------------------------- solves ---
def _mg_ctx(N, m, side="left"):
    import gmres_amd as ga

    c = ga.Context(N, m)
    c.set_precond("mg", side=side)
    c.set_rhs_ones()
    return c


def test_solves_128(oracle):
    """128^2, m = 30, tol 1e-8, the defaults: MGS-R left and right, Householder right, PCG and
    BiCGSTAB (fused drivers), the FP32 basis and CGS2 -- every one to a true residual below
    1e-8; PCG in the restatement's iterations +- 1; right-preconditioned MGS-R in at most
    half the iterations of Chebyshev(8) on (8.2, 0.2)."""
    import gmres_amd as ga

    N, m, tol = 128, 30, 1e-8
    its = {}
    for side in ("left", "right"):
        with _mg_ctx(N, m, side) as c:
            r = ga.gmres_mgsr(c, tol)
            its["mgsr-" + side] = r.iterations
            res = c.true_residual()
            print(f"mgsr {side}: {r.iterations} iterations, true residual {res:.3e}")
            assert res < tol
    with ga.Context(N, m) as c:
        c.set_precond("cheb", (8.2, 0.2), 8, side="right")
        c.set_rhs_ones()
        r = ga.gmres_mgsr(c, tol)
        its["cheb8-right"] = r.iterations
        assert c.true_residual() < tol
    print(its)
    assert 2 * its["mgsr-right"] <= its["cheb8-right"]
    with _mg_ctx(N, m) as c:
        r = ga.gmres_hh(c, tol, precondition="right")
        res = c.true_residual()
        print(f"hh right: {r.iterations} iterations, true residual {res:.3e}")
        assert res < tol
    ref_it = _ref_pcg(N)
    with _mg_ctx(N, m) as c:
        atol = tol * c.rhs_norm()  # the short-recurrence drivers stop on ||r||: the restatement's ||r|| / ||b||
        x, it, rn, _ = ga.pcg(c, tol=atol, max_iter=60)
        res = c.true_residual()
        print(f"pcg: {it} iterations (restatement {ref_it}), true residual {res:.3e}")
        assert res < tol and abs(it - ref_it) <= 1
        c.zero_x()
        x, it, rn, _ = ga.pbicgstab(c, tol=atol, max_iter=60)
        res = c.true_residual()
        print(f"bicgstab: {it} iterations, true residual {res:.3e}")
        assert res < tol
    with _mg_ctx(N, m) as c:
        c.set_basis("f32")
        r = ga.gmres_mgsr(c, tol)
        res = c.true_residual()
        print(f"f32 basis: {r.iterations} iterations, true residual {res:.3e}")
        assert res < tol
    with _mg_ctx(N, m) as c:
        c.set_orth("cgs2")
        r = ga.gmres_mgsr(c, tol)
        res = c.true_residual()
        print(f"cgs2: {r.iterations} iterations, true residual {res:.3e}")
        assert res < tol


def test_pcg_1024():
    """1024^2: PCG to ||r|| / ||b|| < 1e-8 within the CPU table's 11 iterations + 2."""
    import gmres_amd as ga

    with _mg_ctx(1024, 8) as c:
        assert c.mg_info()["sides"] == [1024, 512, 256, 128, 64, 32, 16, 8]
        x, it, rn, _ = ga.pcg(c, tol=1e-8 * c.rhs_norm(), max_iter=40)
        res = c.true_residual()
        print(f"pcg 1024^2: {it} iterations, true residual {res:.3e}")
        assert res < 1e-8 and it <= 13


def test_fortran_plugin_driver():
    """The Fortran plug-in hip_mg end to end (`test_mfp_hip <N> <m> mg`): gmres_mgsr_hip with it
    on the right to a true relative residual of 1e-12, then pcg_hip with it to ||r|| < 1e-10;
    both recognise the plug-in, converge in multigrid's few iterations and return x = 1."""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmres_amd", "lib", "test_mfp_hip")
    out = subprocess.run([exe, "128", "30", "mg"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "multigrid V-cycle on the right" in out.stdout and "Householder" not in out.stdout
    val = lambda key: float([l for l in out.stdout.splitlines() if key in l][0].split(":")[1].split()[0])  # noqa: E731
    assert val("Final residual") < 1e-12
    assert val("Iterations until convergence") <= 20  # 9 to 1e-8 at a rate near 0.1 per iteration
    assert val("Max error L_max") < 1e-9
    assert val("PCG iterations") <= 20
    assert val("PCG residual") < 1e-10
    assert val("PCG max error L_max") < 1e-9


# ---------------------------------------------------------- refusals and state ---
def test_refusals():
    import gmres_amd as ga
    import gmres_amd.solver as S
    from gmres_amd import _native as nat

    L = nat.hip()
    pr = np.array([8.0, 1.0])
    p = pr.ctypes.data_as(nat._dp)
    for N in (127, 14):
        with ga.Context(N, 4) as c:
            assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 2, 2) == nat.GK_ERR_ARG
    with ga.Context(16, 4) as c:
        for degree in (0, 9):
            assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 2, degree) == nat.GK_ERR_ARG
        eq = np.array([3.0, 3.0])
        assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, eq.ctypes.data_as(nat._dp), 2, 2) == nat.GK_ERR_ARG
        assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 1, 2) == nat.GK_ERR_ARG
        info = (ctypes.c_int * nat.GK_MG_INFO_LEN)()
        assert L.gk_mg_info(c.handle, info) == nat.GK_ERR_STATE  # nothing was set
        assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 2, 2) == nat.GK_OK
        assert L.gk_mg_transfer(c.handle, 3, 0, p, p, p) == nat.GK_ERR_ARG
        assert L.gk_mg_transfer(c.handle, 0, 1, p, p, p) == nat.GK_ERR_ARG  # 16 -> 8 has one transfer
    with ga.Context(32, 4, line0=0, nlines=16) as c:  # half the grid
        assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 2, 2) == nat.GK_ERR_STATE
    g = ga.LocalGroup(1)
    try:
        with ga.Context(16, 4) as c:  # a group member
            c.comm_init_local(g, 0, 16)
            assert L.gk_set_precond(c.handle, nat.GK_PREC_MG, p, 2, 2) == nat.GK_ERR_STATE
        with ga.Context(16, 4) as c:  # a communicator on an MG context
            c.set_precond("mg")
            assert L.gk_comm_init_local(c.handle, g.handle, 0, 16) == nat.GK_ERR_STATE
    finally:
        g.close()
    r = torch.zeros(256, dtype=torch.float64, device="cuda")
    z = torch.zeros_like(r)
    with pytest.raises(nat.GkError, match="status -1"):
        S.precond_apply(r, z, 16, kind="mg", params=(8.0, 1.0), degree=2)


def test_state_changes(oracle):
    """MG set twice, then Chebyshev(4): apply is bit-identical to a fresh Chebyshev(4)
    context; mg_info() is mg_plan(N) plus the smoother's degree."""
    import gmres_amd as ga

    N = 48
    v = _data(N * N, N, 7)
    with ga.Context(N, 4) as c:
        c.set_precond("mg")
        info = c.mg_info()
        assert info.pop("degree") == 2
        assert info == ga.mg_plan(N)
        first = c.apply(v, 1)
        c.set_precond("mg", (8.2, 2.0), 3)
        assert c.mg_info()["degree"] == 3
        assert not np.array_equal(c.apply(v, 1), first)
        c.set_precond("mg")
        assert np.array_equal(c.apply(v, 1), first)
        c.set_precond("cheb", (8.2, 0.2), 4)
        after = c.apply(v, 1)
    with ga.Context(N, 4) as c:
        c.set_precond("cheb", (8.2, 0.2), 4)
        fresh = c.apply(v, 1)
    assert np.array_equal(after, fresh)
    assert np.array_equal(fresh, oracle.precond(oracle.PREC_CHEB, v, N, params=(8.2, 0.2), degree=4))
