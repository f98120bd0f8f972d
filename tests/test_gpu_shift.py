"""gk_set_shift on the GPU: the operator A_sigma = A_poisson + sigma I on every path that forms
A t, against its restatement on host arrays (tests/shift_data.py, pinned to the CPU oracle at
sigma = 0 by tests/test_shift_data.py).

The rule: y = fma(fl(4 + sigma), c, -(((W + E) + N) + S)), one rounding; multigrid level l runs
sigma_l = 4^l sigma on the caller's interval moved by sigma_l - sigma.  Every element-wise
stage is a single IEEE operation on both sides, so operator images, preconditioner
applications, transfers and whole V-cycles are compared with np.array_equal.  sigma = 4
makes the diagonal a power of two (8: the product is exact), sigma = 0.37 does not (the fused
rounding is exercised).
"""
import ctypes
import functools
import math
import os
import subprocess
import threading

import numpy as np
import pytest

from tests import general_data as gd
from tests import mg_data
from tests import shift_data as sd

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIGMAS = (4.0, 0.37)
SIZES = (16, 67, 130, 514)
MG_SIZES = (16, 48, 130, 514)
T_CHEB_FUSED, T_RES, T_CHEB_STEN, T_GRAPH, T_SR_TWO, T_RIGHT_FUSED, T_MG_FUSED = 6, 8, 16, 19, 29, 31, 33


def _col(c, k):
    """V(:,k+1) of a context through the device vector API (copy to x)."""
    from gmres_amd import _native as nat

    nat.check(nat.hip().gk_vec_lincomb(c.handle, 0, 0, 2 + k, 0, 0, 0.0, 0.0), "gk_vec_lincomb")
    return c.get_x()


def _vec_apply(c, what, v):
    c.set_x(v)
    c.vec_apply(what, 0, 2)
    return _col(c, 0)


@functools.lru_cache(maxsize=None)
def _v(N, seed=0):
    v = sd.asym(N, 9000 + 31 * N + seed)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _model(N, sg, what):
    """The model's images of _v(N), once per (shape, shift)."""
    v = _v(N)
    pr = (8.2 + sg, 0.2 + sg)
    if what == "A":
        out = sd.stencil(v, N, sg)
    elif what == "cbpr2":
        out = sd.cbpr2(v, N, sg, pr)
    elif what == "A cbpr2":
        out = sd.stencil(_model(N, sg, "cbpr2"), N, sg)
    elif what.startswith("cheb"):
        out = sd.cheb(v, N, sg, pr, int(what[4:]))
    else:
        raise KeyError(what)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ operator ---
@pytest.mark.parametrize("sg", SIGMAS)
@pytest.mark.parametrize("N", SIZES)
def test_operator_paths_bitexact(N, sg):
    """gk_apply(0), gk_vec_apply 0 / 1 / 2 and the preconditioners that carry the stencil: cbpr2
    on the left, cbpr2 on the right fused (k_right_cbpr2) and unfused, Chebyshev(2) and (8) as
    temporal-blocked passes and sweep by sweep.  16: lanes masked; 67: one point per lane;
    130: a wave-window seam at column 128; 514: a second workgroup along i; line-tile seams
    at every size."""
    import gmres_amd as ga

    v = _v(N)
    pr = (8.2 + sg, 0.2 + sg)
    with ga.Context(N, 4) as c:
        assert c.shift == 0.0
        c.set_shift(sg)
        assert c.shift == sg
        assert np.array_equal(c.apply(v, 0), _model(N, sg, "A"))
        assert np.array_equal(_vec_apply(c, 0, v), _model(N, sg, "A"))
        c.set_precond("cbpr2", pr)
        assert np.array_equal(c.apply(v, 1), _model(N, sg, "cbpr2"))
        assert np.array_equal(_vec_apply(c, 1, v), _model(N, sg, "cbpr2"))
        for fused in (1, 0):
            c.tune(T_RIGHT_FUSED, fused)
            assert np.array_equal(_vec_apply(c, 2, v), _model(N, sg, "A cbpr2")), fused
        for deg in (2, 8):
            for fused in (1, 0):
                c.tune(T_CHEB_FUSED, fused)
                c.set_precond("cheb", pr, deg)
                got = c.apply(v, 1)
                assert np.array_equal(got, _model(N, sg, f"cheb{deg}")), (deg, fused, float(np.abs(got - _model(N, sg, f"cheb{deg}")).max()))


@pytest.mark.parametrize("sg", SIGMAS)
@pytest.mark.parametrize("N", SIZES)
def test_poisson5_shift_stateless(N, sg):
    """gk_poisson5_shift on the whole grid, and on lines 5 .. 11 with and without their
    neighbour lines; shift = 0 stays gk_poisson5."""
    import gmres_amd.solver as S

    v = _v(N)
    g = v.reshape(N, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).cuda()  # noqa: E731
    x = dev(v)
    y = torch.zeros_like(x)
    S.poisson5(x, y, N, shift=sg)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), _model(N, sg, "A"))
    xs, lo, hi = dev(g[5:12]), dev(g[4]), dev(g[12])
    ys = torch.zeros_like(xs)
    S.poisson5(xs, ys, N, nlines=7, halo_lo=lo, halo_hi=hi, shift=sg)
    torch.cuda.synchronize()
    assert np.array_equal(ys.cpu().numpy().reshape(7, N), _model(N, sg, "A").reshape(N, N)[5:12])
    S.poisson5(xs, ys, N, nlines=7, shift=sg)
    torch.cuda.synchronize()
    assert np.array_equal(ys.cpu().numpy(), sd.stencil(g[5:12], N, sg))
    S.poisson5(x, y, N)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), sd.stencil(v, N, 0.0))


@pytest.mark.parametrize("sg", SIGMAS)
@pytest.mark.parametrize("N", [130, 514])
def test_in_step_stencil_stage(N, sg):
    """One gk_mgs_step on planted columns with Chebyshev(4) on the left: the pass's stage 0
    forms A_sigma v itself (GK_TUNE_CHEB_STEN 1).  The step agrees with the long-double step
    on the model's operator image w0 = M^-1 A_sigma v within general_data's step bounds, on this
    route and on the stencil launch + pass route (GK_TUNE_CHEB_STEN 0; the two differ in the
    first dot's summation order, test_gpu_kernels.py).  The step's own w is w0 again when put
    back together, sum_i h_i V_i + h_{j+1} v_new: every rounding of the step is relative to
    |w| <= |w0| (two passes of j projections, the norm, the scale: under twenty), so the
    rebuilt vector lies within 64 eps max |w0| of the model's image, element by element."""
    import gmres_amd as ga

    m, j, deg = 3, 2, 4
    pr = (8.2 + sg, 0.2 + sg)
    V = gd.planted_basis(N, j, seed=77 + N)
    w0 = sd.cheb(sd.stencil(V[j - 1], N, sg), N, sg, pr, deg)
    ref = gd.mgs_step_ld(V, w0)
    # A_sigma is well conditioned and Chebyshev(4) on its interval nearly inverts it: w0 is
    # V_{j-1} to within h_{j+1} ~ 1e-3, so the projections cancel most of it.  Their roundings
    # are relative to w0, and the new column is the remainder over h_{j+1}: the column's bound
    # is general_data's 64 eps on max |w0| / h_{j+1} where that exceeds max |v_ref| (without
    # cancellation the two are the same number).
    hb, vb = gd.step_bounds(V, w0, ref[1])
    vb = max(vb, gd.MARGIN * gd.EPS * float(np.max(np.abs(w0))) / float(ref[0][j]))
    for sten in (1, 0):
        with ga.Context(N, m) as c:
            c.tune(T_CHEB_STEN, sten)
            c.set_shift(sg)
            c.set_precond("cheb", pr, deg)
            c.set_rhs_ones()
            c.mgs_cycle_start()
            for k in range(j):
                gd.plant(c, k, V[k])
            assert c.res_info()["cheb_sten"] == sten
            h = c.mgs_step(j)
            vn = gd.read_col(c, j)
            gd.check_step(h, vn, V, w0, ref, f"shift {sg} sten {sten} N={N}", bounds=(hb, vb))
            ld = np.longdouble
            back = (np.asarray(h[:j], dtype=ld) @ np.asarray(V, dtype=ld) + ld(h[j]) * np.asarray(vn, dtype=ld))
            dev = float(np.max(np.abs(back - np.asarray(w0, dtype=ld))))
            lim = gd.MARGIN * gd.EPS * float(np.max(np.abs(w0)))
            print(f"shift {sg} sten {sten} N={N}: max |rebuilt w - w0| {dev:.3e}, bound {lim:.3e}")
            assert dev <= lim


@pytest.mark.parametrize("solver", ["pcg", "pbicgstab"])
def test_short_recurrence_marches(solver):
    """The short-recurrence marches (k_sr_march, k_sr_march2) carry the same diagonal: with
    cbpr2 at sigma = 0.37 the two-level and one-level marches give one history and one x, and
    the solve's own residual is the one k_stencil forms (gk_true_residual)."""
    import gmres_amd as ga

    N, sg, K = 130, 0.37, 12
    b = sd.stencil(_v(N, 1), N, sg)
    outs = []
    for two in (1, 0):
        with ga.Context(N, 8) as c:
            c.tune(T_SR_TWO, two)
            c.set_shift(sg)
            c.set_precond("cbpr2", (8.2 + sg, 0.2 + sg))
            c.set_rhs(b)
            c.zero_x()
            s = ga.SrSolve(c, solver, 0.0, K)
            s.iterate(K)
            ex, done, res = s.status()
            assert ex == K
            h = s.history(ex)
            true = c.true_residual() * c.rhs_norm()
            print(f"{solver} two-level {two}: recurrence ||r|| {res:.6e}, true ||b - A x|| {true:.6e}")
            assert abs(true - res) <= 1e-10 * c.rhs_norm()
            outs.append((h, c.get_x()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------- multigrid ---
def _mgp(sg):
    return (8.0 + sg, 1.0 + sg)


@functools.lru_cache(maxsize=None)
def _model_cycle(N, sg):
    out = sd.mg(_v(N), N, sg, _mgp(sg))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("sg", SIGMAS)
@pytest.mark.parametrize("N", MG_SIZES)
def test_multigrid_bitexact(N, sg):
    """The fused residual-restriction at levels 0 and 1 (gk_mg_transfer what 1: level l runs
    diag = fl(4 + 4^l sigma)), the whole V-cycle with GK_TUNE_MG_FUSED 1 and 0, and nu_c, with
    the shift set before the hierarchy is built and after (the in-place refresh).  514 -> 257:
    the per-sweep smoother on an odd level."""
    import gmres_amd as ga

    v, ref = _v(N), _model_cycle(N, sg)
    sides = mg_data.levels(N)
    for order in ("shift-first", "precond-first"):
        with ga.Context(N, 4) as c:
            if order == "shift-first":
                c.set_shift(sg)
                c.set_precond("mg", _mgp(sg))
            else:
                c.set_precond("mg", _mgp(sg))
                assert c.mg_info()["coarse_degree"] == sd.nu_c(N, 0.0)
                c.set_shift(sg)
            info = c.mg_info()
            assert info["sides"] == sides
            print(f"N={N} sigma={sg} {order}: nu_c {info['coarse_degree']} (sigma = 0: {sd.nu_c(N, 0.0)})")
            assert info["coarse_degree"] == sd.nu_c(N, sg)
            for mgf in (1, 0):
                c.tune(T_MG_FUSED, mgf)
                got = c.apply(v, 1)
                assert np.array_equal(got, ref), (order, mgf, float(np.abs(got - ref).max()))
            c.tune(T_MG_FUSED, 1)
            for level in range(min(2, len(sides) - 1)):
                n = sides[level]
                a, b = sd.asym(n, 100 * N + level), sd.asym(n, 200 * N + level)
                assert np.array_equal(c.mg_transfer(1, level, a, b), sd.resid_restrict(a, b, n, sg * 4.0 ** level)), level
            assert np.array_equal(c.apply(v, 1), ref)  # the transfers left the hierarchy's state alone


# -------------------------------------------------------------------- solves ---
@functools.lru_cache(maxsize=None)
def _model_pcg(N, sg):
    from oracle import oracle as orc

    orc.build()
    return sd.pcg(orc, N, sg, full=True)


def _solve_ctx(N, m, sg, side="left"):
    import gmres_amd as ga

    c = ga.Context(N, m)
    c.set_shift(sg)
    c.set_precond("mg", _mgp(sg), side=side)
    c.set_rhs_ones()
    return c


@pytest.mark.parametrize("sg", [0.01, 1.0])
def test_solves_128(oracle, sg):
    """128^2, b = A_sigma 1, multigrid on (8 + sigma, 1 + sigma): PCG, BiCGSTAB, MGS-R left and
    right and Householder right reach a true relative residual <= 1e-8; PCG in exactly the
    model's iterations; every max |x - 1| within 10 x the model's own at the same iteration
    count (the model: shift_data.pcg / pbicgstab / gmres)."""
    import gmres_amd as ga

    N, m, tol = 128, 30, 1e-8
    ref_it, _, ref_x = _model_pcg(N, sg)
    assert np.array_equal(sd.rhs_ones(N, sg), _rhs_of(N, sg))
    with _solve_ctx(N, m, sg) as c:
        atol = tol * c.rhs_norm()
        x, it, rn, _ = ga.pcg(c, tol=atol, max_iter=60)
        res = c.true_residual()
        e, em = float(np.max(np.abs(x - 1.0))), float(np.max(np.abs(ref_x - 1.0)))
        print(f"sigma {sg} pcg: {it} iterations (model {ref_it}), true residual {res:.3e}, max|x-1| {e:.3e} (model {em:.3e})")
        assert res <= tol and it == ref_it
        assert e <= 10.0 * em
        c.zero_x()
        x, it, rn, _ = ga.pbicgstab(c, tol=atol, max_iter=60)
        res = c.true_residual()
        e, em = float(np.max(np.abs(x - 1.0))), float(np.max(np.abs(sd.pbicgstab(oracle, N, sg, it) - 1.0)))
        print(f"sigma {sg} bicgstab: {it} iterations, true residual {res:.3e}, max|x-1| {e:.3e} (model {em:.3e})")
        assert res <= tol
        assert e <= 10.0 * em
    for what, side in (("mgsr-left", "left"), ("mgsr-right", "right"), ("hh-right", "right")):
        with _solve_ctx(N, m, sg, side if what.startswith("mgsr") else "left") as c:
            r = ga.gmres_mgsr(c, tol) if what.startswith("mgsr") else ga.gmres_hh(c, tol, precondition="right")
            res = c.true_residual()
            assert r.n_cycles == 1
            e = float(np.max(np.abs(r.x - 1.0)))
            em = float(np.max(np.abs(sd.gmres(N, sg, r.iterations, side) - 1.0)))
            print(f"sigma {sg} {what}: {r.iterations} iterations, true residual {res:.3e}, max|x-1| {e:.3e} (model {em:.3e})")
            assert res <= tol
            assert e <= 10.0 * em


def _rhs_of(N, sg):
    """b of set_rhs_ones under the shift, read back through b -> x."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    with ga.Context(N, 4) as c:
        c.set_shift(sg)
        c.set_rhs_ones()
        nat.check(nat.hip().gk_vec_lincomb(c.handle, 0, 0, 1, 0, 0, 0.0, 0.0), "gk_vec_lincomb")  # x = b
        return c.get_x()


def test_pcg_1024_not_slower_than_unshifted():
    """1024^2, sigma = 0.1: PCG to 1e-8 in no more iterations than sigma = 0
    (test_gpu_mg.py::test_pcg_1024's solve, run here beside it)."""
    import gmres_amd as ga

    its = {}
    for sg in (0.0, 0.1):
        with _solve_ctx(1024, 8, sg) as c:
            x, it, rn, _ = ga.pcg(c, tol=1e-8 * c.rhs_norm(), max_iter=40)
            res = c.true_residual()
            print(f"pcg 1024^2 sigma {sg}: {it} iterations, true residual {res:.3e}")
            assert res <= 1e-8
            its[sg] = it
    assert its[0.1] <= its[0.0]


# --------------------------------------------------------------------- state ---
def test_argument_errors():
    import gmres_amd as ga
    from gmres_amd import _native as nat

    L = nat.hip()
    with ga.Context(16, 4) as c:
        c.set_shift(0.25)
        for bad in (-1.0, math.nan, math.inf, -math.inf, 1e13):
            assert L.gk_set_shift(c.handle, bad) == nat.GK_ERR_ARG, bad
            assert c.shift == 0.25
        assert L.gk_set_shift(c.handle, 1e12) == nat.GK_OK
        assert L.gk_get_shift(c.handle, None) == nat.GK_ERR_ARG
    x = torch.zeros(256, dtype=torch.float64, device="cuda")
    y = torch.zeros_like(x)
    for bad in (-1.0, math.nan, math.inf, 1e13):
        assert L.gk_poisson5_shift(16, 16, bad, x.data_ptr(), None, None, y.data_ptr(), None) == nat.GK_ERR_ARG


def test_shift_ends_an_open_cycle():
    import gmres_amd as ga
    from gmres_amd import _native as nat

    with ga.Context(48, 4) as c:
        c.set_rhs(sd.asym(48, 5))
        c.mgs_cycle_start()
        c.mgs_step(1)
        c.set_shift(0.37)
        h = np.zeros(3)
        assert nat.hip().gk_mgs_step(c.handle, 2, h.ctypes.data_as(nat._dp)) == nat.GK_ERR_STATE
        c.mgs_cycle_start()
        c.mgs_step(1)
        c.set_shift(0.37)  # the same value ends it too
        assert nat.hip().gk_mgs_step(c.handle, 2, h.ctypes.data_as(nat._dp)) == nat.GK_ERR_STATE


def _cycle_columns(c, m):
    c.zero_x()
    beta = c.mgs_cycle_start()
    return [np.array([beta])] + [c.mgs_step(j) for j in range(1, m + 1)]


@pytest.mark.parametrize("prec", ["cbpr2", "cheb", "mg"])
def test_no_stale_graph_after_shift(prec):
    """Captured launch-path steps (GK_TUNE_GRAPH 1, GK_TUNE_RES 0) hold diag by value: after
    two cycles at sigma = 0 (capture, replay) and gk_set_shift(0.37), a cycle's Hessenberg
    columns are those of a fresh context at 0.37, bit for bit; and back at 0, the first's."""
    import gmres_amd as ga

    N, m, sg = 48, 5, 0.37
    b = sd.asym(N, 6)

    def setup(c, s):
        c.tune(T_GRAPH, 1)
        c.tune(T_RES, 0)
        if s is not None:
            c.set_shift(s)
        if prec == "mg":
            c.set_precond("mg")
        else:
            c.set_precond(prec, (8.2, 0.2), 4)
        c.set_rhs(b)

    with ga.Context(N, m) as c:
        setup(c, None)
        first = _cycle_columns(c, m)
        again = _cycle_columns(c, m)
        c.set_shift(sg)
        moved = _cycle_columns(c, m)
        moved2 = _cycle_columns(c, m)
        c.set_shift(0.0)
        back = _cycle_columns(c, m)
    with ga.Context(N, m) as c:
        setup(c, sg)
        fresh = _cycle_columns(c, m)
    for a_, b_ in zip(first, again):
        assert np.array_equal(a_, b_)
    assert not all(np.array_equal(a_, b_) for a_, b_ in zip(first, moved))
    for j, (a_, b_) in enumerate(zip(moved, fresh)):
        assert np.array_equal(a_, b_), (j, a_, b_)
    for a_, b_ in zip(moved2, fresh):
        assert np.array_equal(a_, b_)
    for a_, b_ in zip(back, first):
        assert np.array_equal(a_, b_)


@pytest.mark.parametrize("solver", ["pcg", "pbicgstab"])
def test_no_stale_sr_graph_after_shift(solver):
    """A chunked gk_sr_* solve (its 16-iteration graph captured at sigma = 0), restarted after
    gk_set_shift(0.37): history and x of a fresh context at 0.37; the running solve is ended."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    N, K, sg = 48, 20, 0.37
    b = sd.asym(N, 8)

    def run(c):
        c.zero_x()
        s = ga.SrSolve(c, solver, 0.0, K)
        s.iterate(K)
        ex, done, res = s.status()
        assert ex == K
        return s, s.history(ex), c.get_x()

    with ga.Context(N, 8) as c:
        c.set_precond("mg")
        c.set_rhs(b)
        s, h0, x0 = run(c)
        c.set_shift(sg)
        assert nat.hip().gk_sr_iterate(c.handle, 1) == nat.GK_ERR_STATE
        _, h1, x1 = run(c)
    with ga.Context(N, 8) as c:
        c.set_shift(sg)
        c.set_precond("mg")
        c.set_rhs(b)
        _, hf, xf = run(c)
    assert not np.array_equal(h0, h1)
    assert np.array_equal(h1, hf) and np.array_equal(x1, xf)


def test_shift_zero_is_the_default_solve():
    import gmres_amd as ga

    N, m = 48, 10
    b = sd.asym(N, 9)

    def solve(c):
        c.set_precond("cheb", (8.2, 0.2), 4)
        c.set_rhs(b)
        c.zero_x()
        return ga.gmres_mgsr(c, 1e-12, want_hist=True)

    with ga.Context(N, m) as c:
        ref = solve(c)
    with ga.Context(N, m) as c:
        c.set_shift(0.37)
        other = solve(c)
        c.set_shift(0.0)
        got = solve(c)
    assert not np.array_equal(other.x, ref.x)
    assert np.array_equal(got.x, ref.x) and np.array_equal(got.hist_res, ref.hist_res)
    assert np.array_equal(got.final_err, ref.final_err) and got.iterations == ref.iterations


def test_lanczos_bounds_move_by_the_shift():
    import gmres_amd as ga

    N, sg = 64, 0.37
    with ga.Context(N, 8) as c:
        lo0, hi0 = c.lanczos_bounds(30)
        c.set_shift(sg)
        lo1, hi1 = c.lanczos_bounds(30)
    print(f"lanczos: ({lo0!r}, {hi0!r}) -> ({lo1!r}, {hi1!r})")
    assert abs(lo1 - (lo0 + sg)) <= 1e-9 * abs(lo0 + sg)
    assert abs(hi1 - (hi0 + sg)) <= 1e-9 * abs(hi0 + sg)


# --------------------------------------------------------------------- ranks ---
def test_three_ranks_match_one():
    """Three row-block ranks on one GPU (in-process group), N = 48, sigma = 0.37: every rank's
    rows of A_sigma v and of Chebyshev(2) are the one-rank result bit for bit."""
    import gmres_amd as ga

    N, sg = 48, 0.37
    v = _v(48, 2)
    pr = (8.2 + sg, 0.2 + sg)
    with ga.Context(N, 4) as c:
        c.set_shift(sg)
        c.set_precond("cheb", pr, 2)
        one = (c.apply(v, 0), c.apply(v, 1))
    assert np.array_equal(one[0], sd.stencil(v, N, sg)) and np.array_equal(one[1], sd.cheb(v, N, sg, pr, 2))
    parts = ga.slab_partition(N, 3)
    ml = max(nl for _, nl in parts)
    g = ga.LocalGroup(3)
    ctxs = [ga.Context(N, 4, line0=l0, nlines=nl) for l0, nl in parts]
    for r, c in enumerate(ctxs):
        c.comm_init_local(g, r, ml)
    out, err = [None] * 3, []

    def work(r):
        try:
            c = ctxs[r]
            l0, nl = parts[r]
            mine = v[l0 * N:(l0 + nl) * N]
            c.set_shift(sg)
            c.set_precond("cheb", pr, 2)
            out[r] = (c.apply(mine, 0), c.apply(mine, 1))
        except Exception as e:  # pragma: no cover - reported below
            err.append(e)

    th = [threading.Thread(target=work, args=(r,)) for r in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    for c in ctxs:
        c.close()
    g.close()
    assert not err, err
    for k in (0, 1):
        assert np.array_equal(np.concatenate([o[k] for o in out]), one[k]), k


# ------------------------------------------------------------------- Fortran ---
def test_fortran_driver_shift():
    """`test_mfp_hip 64 20 shift`: hip_set_shift(0.5), b = (A + 0.5 I) 1 through hip_poisson5,
    gmres_mgsr_hip with hip_mg on the right and pcg_hip with it on (8.5, 1.5)."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmres_amd", "lib", "test_mfp_hip")
    out = subprocess.run([exe, "64", "20", "shift"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shifted" in out.stdout
    errs = [float(l.split(":")[1].split()[0]) for l in out.stdout.splitlines() if "ax error L_max" in l]
    assert len(errs) == 2 and max(errs) < 1e-8, errs
