"""Right-preconditioned MGS-R GMRES(m) on the GPU (gk_set_precond_side):
w = A M^-1 v_j, x += M^-1 (V y), so final_err is the true relative residual.

The operator A M^-1 v is checked bit for bit against the CPU oracle on both of
its routes (the two-level march k_right_cbpr2 and the preconditioner + stencil
launches), the solves against the host restatement tests/right_gmres_host.py."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from tests.right_gmres_host import CASES, TOL, case_id, first_dot_host, host_solve

pytestmark = pytest.mark.gpu

PARAMS = (8.2, 0.2)
STENCIL_BLOCKS = 2  # GK_TUNE_STENCIL_BLOCKS
# the kinds of the operator test: (id, preconditioner, degree, GK_TUNE_RIGHT_FUSED)
ROUTES = [("cbpr2-fused", "cbpr2", 1, 1), ("cbpr2-two-launch", "cbpr2", 1, 0), ("cheb3", "cheb", 3, 1),
          ("cheb8", "cheb", 8, 1), ("identity", "identity", 1, 1)]
# N: 2, 3, 5 tiny; 64 VEC 2, half a wave; 65 VEC 1, two waves, the second holding one lane;
# 128 exactly one wave, VEC 2; 130 wave seam, VEC 2; 257 VEC 1, two x-blocks, the second
# holding one point; 514 VEC 2, two x-blocks, the second holding two points
SHAPES = [2, 3, 5, 64, 65, 128, 130, 257, 514]


def _kind(oracle, prec):
    return {"cbpr2": oracle.PREC_CBPR2, "cheb": oracle.PREC_CHEB, "identity": oracle.PREC_IDENTITY}[prec]


def _copy(c, dst, src):
    from gmres_amd import _native as nat

    nat.check(nat.hip().gk_vec_lincomb(c.handle, 0, dst, src, 0, 0, 0.0, 0.0), "gk_vec_lincomb")  # GK_LC_COPY


def _apply_right(c, v):
    """A M^-1 v through the device vector API: v -> x -> column 0, vec_apply(2) into
    column 1, column 1 -> x -> host."""
    c.set_x(v)
    _copy(c, 2, 0)
    c.vec_apply(2, 2, 3)
    _copy(c, 0, 3)
    return c.get_x()


_vecs: dict = {}


def _rand(N):
    if N not in _vecs:
        _vecs[N] = np.random.default_rng(1000 + N).standard_normal(N * N)
    return _vecs[N]


_refs: dict = {}


def _ref_right(oracle, N, prec, degree):
    """oracle.stvec(oracle.precond(kind, v)), once per (N, kind)."""
    key = (N, prec, degree)
    if key not in _refs:
        _refs[key] = oracle.stvec(oracle.precond(_kind(oracle, prec), _rand(N), N, params=PARAMS, degree=degree), N)
    return _refs[key]


# ------------------------------------------------------------------ 1. operator --

@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_right_operator_bitexact(oracle, N, route):
    import gmres_amd as ga
    from gmres_amd import _native as nat

    _, prec, degree, fused = route
    with ga.Context(N, 4) as c:
        c.tune(nat.GK_TUNE_RIGHT_FUSED, fused)
        c.set_precond(prec, PARAMS, degree)
        out = _apply_right(c, _rand(N))
    assert np.array_equal(out, _ref_right(oracle, N, prec, degree))


@pytest.mark.parametrize("N,blocks", [(64, 0), (64, 3), (64, 1), (130, 0), (130, 3), (130, 1)])
def test_right_operator_line_tiles(oracle, N, blocks):
    """The march across line-tile seams: GK_TUNE_STENCIL_BLOCKS 0 (default) gives
    JT = 1, every line a tile; 3 gives ragged tiles (N = 64: JT = 22, tiles of 22 /
    22 / 20 lines; N = 130: 44 / 44 / 42); 1 the longest marches (N = 64: one tile
    of all lines; N = 130: JT capped at 64, tiles of 64 / 64 / 2)."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    with ga.Context(N, 4) as c:
        c.tune(STENCIL_BLOCKS, blocks)
        c.set_precond("cbpr2", PARAMS)
        c.tune(nat.GK_TUNE_RIGHT_FUSED, 1)
        out = _apply_right(c, _rand(N))
    assert np.array_equal(out, _ref_right(oracle, N, "cbpr2", 1))


# ------------------------------------------------------- 2. the fused route runs --

@pytest.mark.parametrize("fused,launches", [(1, 1), (0, 2)])
def test_right_step_stencil_launches(fused, launches):
    """One Arnoldi step at N = 128, cbpr2, side right: ONE launch under
    GK_KID_STENCIL with the march, two (cbpr2 sweep + stencil) without."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    with ga.Context(128, 6) as c:
        c.tune(nat.GK_TUNE_RIGHT_FUSED, fused)
        c.set_precond("cbpr2", PARAMS, side="right")
        c.set_rhs_ones()
        c.mgs_cycle_start()
        c.profile(True)
        c.profile_reset()
        c.mgs_step(1)
        n = c.profile_read()["stencil"][1]
        c.profile(False)
    assert n == launches


# ------------------------------------------------- 3. step with the dot epilogue --

@pytest.mark.parametrize("N", [65, 130, 514])
def test_right_step_dot_epilogue(oracle, N):
    """Steps 1..4 with the march against the two-launch route: the same w bit for
    bit and the dot on the same workgroup grid, checked to the tolerances of two
    routes that may differ in the dot's summation (test_fused_chebyshev_dot_epilogue_step).
    Step 1's first dot against the host: within 1e-13 sum |w_i v_i|."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    res = {}
    for fused in (1, 0):
        with ga.Context(N, 10) as c:
            c.tune(nat.GK_TUNE_RIGHT_FUSED, fused)
            c.set_precond("cbpr2", PARAMS, side="right")
            c.set_rhs_ones()
            c.mgs_cycle_start()
            cols = [c.mgs_step(j) for j in range(1, 5)]
            _copy(c, 0, 2 + 4)
            res[fused] = (cols, c.get_x())
    for a, b in zip(res[1][0], res[0][0]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-15)
    assert np.allclose(res[1][1], res[0][1], rtol=1e-10, atol=1e-14)
    h0, scale = first_dot_host(oracle, N, "cbpr2")
    for fused in (1, 0):
        dev = res[fused][0][0][0]
        print(f"N={N} fused={fused}: H(1,1) {dev!r} host {h0!r} |diff| {abs(dev - h0):.3e} bound {1e-13 * scale:.3e}")
        assert abs(dev - h0) <= 1e-13 * scale


# ------------------------------------------------ 4, 5. histories and the gap ----

def _dev_solve(case, side, max_cycles=None, fused=1):
    import gmres_amd as ga
    from gmres_amd import _native as nat

    N, m, prec, degree, cap = case
    cap = cap if max_cycles is None else max_cycles
    with ga.Context(N, m) as c:
        c.tune(nat.GK_TUNE_RIGHT_FUSED, fused)
        c.set_precond(prec, PARAMS, degree or 8, side=side)
        c.set_rhs_ones()
        return ga.gmres_mgsr(c, tol=TOL, variant=ga.MGSR_MF, max_cycles=min(cap, 1000), want_hist=True)


def _gap_dev(r):
    """max over cycles of |hist_ferr[c, n_out_c - 1] / hist_res[c] - 1|; n_out_c is the
    last step the cycle wrote (a cycle's unwritten steps stay zero)."""
    g = 0.0
    for c in range(r.n_cycles):
        n_out = int(np.count_nonzero(r.hist_ferr[c]))
        g = max(g, abs(r.hist_ferr[c, n_out - 1] / r.hist_res[c] - 1.0))
    return g


def _cap(case):
    return 6 if case[0] == 130 else None  # the unconverged case: six cycles of it


_dev_runs: dict = {}


def _dev_right(case):
    if case not in _dev_runs:
        _dev_runs[case] = _dev_solve(case, "right", _cap(case))
    return _dev_runs[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_right_histories_match_host(oracle, case):
    """hist_res per cycle and the last cycle's final_err within rtol 1e-5 / atol 1e-13
    (the MGS-R contract of DESIGN.md 4.3), the same cycle count, n_out within one,
    and the solution: |x - 1| < 1e-6 where the host run converged.  The 130^2 case is
    cut after six cycles, far from converged (the host's own x is 0.79 from 1 there),
    so its x is held to the host's x instead, to the same 1e-6."""
    h = host_solve(oracle, case, "right", _cap(case))
    r = _dev_right(case)
    print(f"{case_id(case)}: cycles dev {r.n_cycles} host {h.n_cycles}, n_out dev {r.n_out} host {h.n_out}, "
          f"hist_res dev {r.hist_res.tolist()} host {h.hist_res.tolist()}")
    assert r.n_cycles == h.n_cycles
    assert np.allclose(r.hist_res, h.hist_res, rtol=1e-5, atol=1e-13)
    assert abs(r.n_out - h.n_out) <= 1
    k = min(r.n_out, h.n_out)
    assert np.allclose(r.final_err[:k], h.final_err[:k], rtol=1e-5, atol=1e-13)
    assert np.allclose(r.hist_ferr[-1, :k], h.hist_ferr[-1, :k], rtol=1e-5, atol=1e-13)
    converged = h.final_err[h.n_out - 1] < TOL
    err = np.max(np.abs(r.x - (1.0 if converged else h.x)))
    print(f"{case_id(case)}: converged {converged}, max |x - {'1' if converged else 'x_host'}| {err:.3e}")
    assert err < 1e-6


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_right_estimate_is_the_true_residual(oracle, case):
    """The point of the feature: at the end of every cycle the stopping quantity is
    the true relative residual.  The gap is rounding noise (loss of orthogonality over
    the residual) and depends on the summation order: a decade over the host's own
    figure, floor 1e-9.  Control: the same solve on the left is off by more than 10 %."""
    gap_host = host_solve(oracle, case, "right", _cap(case)).gap()
    gap_dev = _gap_dev(_dev_right(case))
    gap_left = _gap_dev(_dev_solve(case, "left", _cap(case)))
    print(f"{case_id(case)}: gap_dev {gap_dev:.3e} gap_host {gap_host:.3e} left gap_dev {gap_left:.3e}")
    assert gap_dev <= max(10.0 * gap_host, 1e-9)
    assert gap_left > 0.1


# ------------------------------------------------------------------ 6. identity --

def test_right_identity_is_left():
    """With the identity preconditioner the two sides run the same launches."""
    import gmres_amd as ga

    res = {}
    for side in ("right", "left"):
        with ga.Context(64, 30) as c:
            c.set_precond("identity", side=side)
            c.set_rhs_ones()
            res[side] = ga.gmres_mgsr(c, tol=1e-15, variant=ga.MGSR_MF, max_cycles=3, want_hist=True)
    a, b = res["right"], res["left"]
    assert a.n_cycles == b.n_cycles == 3
    assert np.array_equal(a.hist_res, b.hist_res)
    assert np.array_equal(a.hist_ferr, b.hist_ferr)
    assert np.array_equal(a.x, b.x)


# --------------------------------------------------------------------- 7. slabs --

def _group_right(N, m, nranks, max_cycles):
    """One host thread per rank over the in-process communicator (the pattern of
    tests/test_gpu_multirank.py): local collectives only, no device exchange."""
    import gmres_amd as ga

    parts = ga.slab_partition(N, nranks)
    ml = max(nl for _, nl in parts)
    g = ga.LocalGroup(nranks)
    ctxs = [ga.Context(N, m, device=0, line0=l0, nlines=nl) for l0, nl in parts]
    for r, c in enumerate(ctxs):
        c.comm_init_local(g, r, ml)
    out, err = [None] * nranks, []

    def work(r):
        try:
            c = ctxs[r]
            c.set_precond("cbpr2", PARAMS, side="right")
            c.set_rhs_ones()
            out[r] = ga.gmres_mgsr(c, tol=TOL, variant=ga.MGSR_MF, max_cycles=max_cycles, want_hist=True)
        except Exception as e:  # pragma: no cover - reported below
            err.append(e)

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not err, err
    assert not any(t.is_alive() for t in th)
    for c in ctxs:
        c.close()
    g.close()
    return out


def test_right_slabs_match_single_rank():
    import gmres_amd as ga

    N, m, cyc = 64, 12, 2
    with ga.Context(N, m) as c:
        c.set_precond("cbpr2", PARAMS, side="right")
        c.set_rhs_ones()
        ref = ga.gmres_mgsr(c, tol=TOL, variant=ga.MGSR_MF, max_cycles=cyc, want_hist=True)
    hist = {}
    for nranks in (2, 3):
        res = _group_right(N, m, nranks, cyc)
        assert len({(r.n_out, r.n_cycles) for r in res}) == 1
        assert np.array_equal(res[0].hist_res, res[-1].hist_res)
        hist[nranks] = res[0].hist_res
        print(f"{nranks} ranks: hist_res {hist[nranks].tolist()} single {ref.hist_res.tolist()}")
        assert len(hist[nranks]) == len(ref.hist_res) == cyc
        assert np.allclose(hist[nranks], ref.hist_res, rtol=1e-5, atol=1e-13)
    assert np.allclose(hist[2], hist[3], rtol=1e-5, atol=1e-13)


# ---------------------------------------------------------------- 8. rejections --

def test_right_rejections_and_switch_back():
    import gmres_amd as ga
    from gmres_amd import _native as nat

    L = nat.hip()
    d = ctypes.c_double()
    hcol = np.zeros(12)
    hp = hcol.ctypes.data_as(nat._dp)

    def default_solve(c):
        c.set_precond("cbpr2", PARAMS)
        c.set_rhs_ones()
        return ga.gmres_mgsr(c, tol=1e-15, max_cycles=3, want_hist=True)

    with ga.Context(64, 10) as c:
        c.set_precond("cbpr2", PARAMS, side="right")
        c.set_rhs_ones()
        # Householder and the short-recurrence solvers stay left-only
        assert L.gk_hh_cycle_start(c.handle, 1, ctypes.byref(d)) == nat.GK_ERR_STATE
        assert "left only" in nat.last_error()
        assert L.gk_sr_start(c.handle, nat.GK_SR_PCG, 1e-9, 10) == nat.GK_ERR_STATE
        assert "left only" in nat.last_error()
        assert L.gk_sr_start(c.handle, nat.GK_SR_BICGSTAB, 1e-9, 10) == nat.GK_ERR_STATE
        # an unknown side
        assert L.gk_set_precond_side(c.handle, 2) == nat.GK_ERR_ARG
        # setting the side ends the open cycle
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        assert L.gk_set_precond_side(c.handle, nat.GK_SIDE_LEFT) == nat.GK_OK
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        assert L.gk_set_precond_side(c.handle, nat.GK_SIDE_RIGHT) == nat.GK_OK
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        # back on the left: a default solve is the one of a fresh context, bit for bit
        back = default_solve(c)
    with ga.Context(64, 10) as c:
        fresh = default_solve(c)
    assert np.array_equal(back.hist_res, fresh.hist_res)
    assert np.array_equal(back.hist_ferr, fresh.hist_ferr)
    assert np.array_equal(back.x, fresh.x)
    assert np.array_equal(back.v_err, fresh.v_err)


# ------------------------------------------------------------ Fortran drop-in ----

def test_right_fortran_dropin():
    """gmres_mgsr_hip(..., side=GK_SIDE_RIGHT) through the reference's driver
    (`test_mfp_hip <N> <m> right`: the MGS-R solve alone, tol 1e-15): it converges,
    to x = 1."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmres_amd", "lib",
                       "test_mfp_hip")
    out = subprocess.run([exe, "48", "20", "right"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MGSR Chebyshev on the right" in out.stdout and "Householder" not in out.stdout
    val = lambda key: float([l for l in out.stdout.splitlines() if key in l][0].split(":")[1].split()[0])  # noqa: E731
    print(out.stdout)
    assert val("Final residual") < 1e-15
    assert val("Max error L_max") < 1e-9
