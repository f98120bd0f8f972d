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
@pytest.mark.parametrize("N,level", [(16, 0), (20, 0), (130, 0), (514, 0), (48, 0), (48, 1)])
def test_transfers_bitexact(oracle, N, level):
    """gk_mg_transfer what 0 / 1 / 2 against numpy.  16: lanes masked; 20: a coarse grid of
    10; 130: a wave seam at fine column 128 and several line tiles; 514: two points in a
    second workgroup along i, coarse 257 odd; 48: also level 1 -> 2 (24 -> 12)."""
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
@pytest.mark.parametrize("N", [16, 48, 100, 130, 514])
def test_vcycle_bitexact(oracle, N):
    """c.apply(v, 1) against the restatement: degrees 1..3, two intervals, and the four
    routes GK_TUNE_MG_FUSED x GK_TUNE_CHEB_FUSED -- one result.  gk_vec_apply(1) and (2)
    likewise, the latter composed with the oracle's stencil."""
    import gmres_amd as ga

    with ga.Context(N, 4) as c:
        for params in ((8.0, 1.0), (8.2, 2.0)):
            for degree in (1, 2, 3):
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
