"""Right-preconditioned Householder GMRES(m) on the GPU (GK_HH_PREC_RIGHT): w = b - A x at
the cycle start, w = A M^-1 v_j in a step, x += M^-1 (P_1..P_n [y;0]) at the cycle's end, so
final_err is the true relative residual as with the MGS-R cycle on a right-sided context.

The single step is held to a long-double step on planted reflectors (tests/hh_right_data.py),
the solves to the MGS-R solve of the same Krylov space and to gk_true_residual, and the
one-launch update (the cbpr2 sweep with an accumulating output) to the two-launch route bit
for bit."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from tests import hh_data as hd
from tests import hh_right_data as hr
from tests.general_data import plant
from tests.right_gmres_host import TOL, host_solve

pytestmark = pytest.mark.gpu

PARAMS = (8.2, 0.2)
T_RES, T_R2, T_SHARE, T_TMO, T_WONLY, T_HH_FUSE, T_PC, T_RIGHT_FUSED = 8, 9, 10, 11, 13, 15, 21, 31
RIGHT = 2  # GK_HH_PREC_RIGHT


def _right_ctx(N, m, prec="cbpr2", degree=8, side="left", fused=1):
    import gmres_amd as ga

    c = ga.Context(N, m)
    c.tune(T_RIGHT_FUSED, fused)
    c.set_precond(prec, PARAMS, degree, side=side)
    c.set_rhs_ones()
    return c


# ------------------------------------------------------------------- 1. accepts --

def test_right_value_is_accepted_and_the_others_keep_their_meaning():
    from gmres_amd import _native as nat

    L = nat.hip()
    assert (nat.GK_HH_PREC_NONE, nat.GK_HH_PREC_LEFT, nat.GK_HH_PREC_RIGHT) == (0, 1, RIGHT)
    d = ctypes.c_double()
    hcol = np.zeros(12)
    hp = hcol.ctypes.data_as(nat._dp)
    with _right_ctx(64, 10, side="right") as c:
        # the new value runs on a right-sided context; the left one is still refused there
        assert L.gk_hh_cycle_start(c.handle, RIGHT, ctypes.byref(d)) == nat.GK_OK, nat.last_error()
        assert L.gk_hh_step(c.handle, 1, RIGHT, hp) == nat.GK_OK, nat.last_error()
        assert np.all(np.isfinite(hcol[:2])) and hcol[1] != 0.0
        # a left step inside a right cycle: refused here for the side ...
        assert L.gk_hh_step(c.handle, 2, 1, hp) == nat.GK_ERR_STATE
        assert L.gk_hh_cycle_start(c.handle, 1, ctypes.byref(d)) == nat.GK_ERR_STATE
        assert "left only" in nat.last_error()
        assert L.gk_hh_cycle_start(c.handle, 3, ctypes.byref(d)) == nat.GK_ERR_ARG
        assert L.gk_hh_cycle_start(c.handle, -1, ctypes.byref(d)) == nat.GK_ERR_ARG
    with _right_ctx(64, 10, side="left") as c:
        # ... and on a left-sided context for the cycle it was opened with
        assert L.gk_hh_cycle_start(c.handle, RIGHT, ctypes.byref(d)) == nat.GK_OK, nat.last_error()
        assert L.gk_hh_step(c.handle, 1, RIGHT, hp) == nat.GK_OK, nat.last_error()
        assert L.gk_hh_step(c.handle, 2, 1, hp) == nat.GK_ERR_STATE
        assert "cycle started with 2" in nat.last_error()
        assert L.gk_hh_step(c.handle, 2, 0, hp) == nat.GK_ERR_STATE
        assert L.gk_hh_step(c.handle, 2, 3, hp) == nat.GK_ERR_ARG
        assert L.gk_hh_step_async(c.handle, 2, 3) == nat.GK_ERR_ARG
        assert L.gk_hh_step(c.handle, 2, RIGHT, hp) == nat.GK_OK, nat.last_error()
        # 1 keeps running on the left, and a right step does not fit its cycle
        assert L.gk_hh_cycle_start(c.handle, 1, ctypes.byref(d)) == nat.GK_OK, nat.last_error()
        assert L.gk_hh_step(c.handle, 1, 1, hp) == nat.GK_OK, nat.last_error()
        assert L.gk_hh_step(c.handle, 2, RIGHT, hp) == nat.GK_ERR_STATE
        # the FP32 basis stays MGS-R only
        c.set_basis("f32")
        assert L.gk_hh_cycle_start(c.handle, RIGHT, ctypes.byref(d)) == nat.GK_ERR_STATE
        assert "MGS-R only" in nat.last_error()
        assert L.gk_hh_step_async(c.handle, 1, RIGHT) == nat.GK_ERR_STATE


# ------------------------------------------ 2. final_err is the true residual ----

def _gap(r):
    """max over cycles of |final_err(n_out) / true relative residual - 1| (a cycle's
    unwritten steps stay zero)."""
    g = 0.0
    for c in range(r.n_cycles):
        n_out = int(np.count_nonzero(r.hist_ferr[c]))
        g = max(g, abs(r.hist_ferr[c, n_out - 1] / r.hist_res[c] - 1.0))
    return g


@pytest.mark.parametrize("prec,degree", [("cbpr2", 0), ("cheb", 4)], ids=["cbpr2", "cheb4"])
def test_right_estimate_is_the_true_residual(oracle, prec, degree):
    """N = 64, m = 10, three cycles: after each cycle's update the last |g(j+1)| / ||b|| is
    gk_true_residual, to the tolerance test_gpu_right_precond.py holds the MGS-R cycle to -- a
    decade over the gap of the host's own right-preconditioned solve, floor 1e-9.  Control: the
    same Householder solve on the left is off by more than 10 %."""
    import gmres_amd as ga

    case = (64, 10, prec, degree, 3)
    gap_host = host_solve(oracle, case, "right").gap()
    runs = {}
    for mode in ("right", True):
        with _right_ctx(64, 10, prec, degree or 8) as c:
            runs[mode] = ga.gmres_hh(c, tol=TOL, precondition=mode, max_cycles=3, want_hist=True)
    r = runs["right"]
    assert r.n_cycles == 3
    gap_dev, gap_left = _gap(r), _gap(runs[True])
    print(f"{prec}{degree or ''}: est {[r.hist_ferr[c, np.count_nonzero(r.hist_ferr[c]) - 1] for c in range(3)]} "
          f"true {r.hist_res.tolist()} gap_dev {gap_dev:.3e} gap_host {gap_host:.3e} left gap {gap_left:.3e}")
    assert gap_dev <= max(10.0 * gap_host, 1e-9)
    assert gap_left > 0.1


# ---------------------------------------- 3. the Krylov space of MGS-R right ----

_hh_runs: dict = {}


def _hh_right_run(N, m, cycles=4, tol=1e-15):
    """gmres_hh(.., "right") with cbpr2, once per shape (test 8 reads the 64 / 10 run to
    convergence)."""
    import gmres_amd as ga

    key = (N, m, cycles, tol)
    if key not in _hh_runs:
        with _right_ctx(N, m) as c:
            _hh_runs[key] = ga.gmres_hh(c, tol=tol, precondition="right", max_cycles=cycles, want_hist=True)
    return _hh_runs[key]


@pytest.mark.parametrize("N,m", [(64, 10), (64, 20), (96, 10), (96, 20)])
def test_right_matches_mgsr_right(N, m):
    """Four cycles: the true residual after every cycle against MGS-R on a right-sided
    context -- the same Krylov spaces, so the same minimal residuals (rtol 1e-5, atol 1e-13:
    the history contract of DESIGN.md 4.3)."""
    import gmres_amd as ga

    r = _hh_right_run(N, m)
    with _right_ctx(N, m, side="right") as c:
        ref = ga.gmres_mgsr(c, tol=1e-15, variant=ga.MGSR_MF, max_cycles=4, want_hist=True)
    print(f"N={N} m={m}: hh right {r.hist_res.tolist()} mgsr right {ref.hist_res.tolist()}")
    assert r.n_cycles == ref.n_cycles == 4
    assert np.allclose(r.hist_res, ref.hist_res, rtol=1e-5, atol=1e-13)


# ------------------------------------------------------------------ 4. identity --

def test_right_identity_is_unpreconditioned():
    """With the identity preconditioner GK_HH_PREC_RIGHT runs the launches of GK_HH_PREC_NONE."""
    import gmres_amd as ga

    res = {}
    for mode in ("right", False):
        with _right_ctx(64, 20, "identity") as c:
            res[mode] = ga.gmres_hh(c, tol=1e-15, precondition=mode, midcycle_exit=False, max_cycles=3,
                                    want_hist=True)
    a, b = res["right"], res[False]
    assert a.n_cycles == b.n_cycles == 3
    assert np.array_equal(a.hist_res, b.hist_res)
    assert np.array_equal(a.hist_ferr, b.hist_ferr)
    assert np.array_equal(a.final_err, b.final_err)
    assert np.array_equal(a.x, b.x)


# --------------------------------------- 5. one step against a long-double step --

def _planted_right(N, m, tunes):
    """A context with a GK_HH_PREC_RIGHT cycle open (cbpr2) and hh_data.reflectors(N, m) planted."""
    return hd.hh_open(N, m, tunes, precondition=RIGHT)


def _steps(oracle, N, m, tunes, what):
    out = []
    with _planted_right(N, m, tunes) as c:
        plan = c.res_info(hh=True)
        for j in hr.js(m):
            h, p = hd.hh_dev_step(c, j, RIGHT)
            if j < m:
                plant(c, j, hd.reflectors(N, m)[j])
            hd.check_hh_step(h, p, hr.reference(oracle, N, j, m), j, f"{what} N={N} j={j}", plan=plan)
            out.append((h, p))
    return out, plan


@pytest.mark.parametrize("hh_fuse", [1, 0])
@pytest.mark.parametrize("N", hr.SHAPES)
def test_right_step_on_planted_reflectors(oracle, N, hh_fuse):
    """gk_hh_step(j, GK_HH_PREC_RIGHT), j = 1, 3, m, on planted reflectors within the bounds of
    test_gpu_hh_step_known_answer.py of the long-double step whose operator is A M^-1, with the
    one-launch operator (GK_TUNE_RIGHT_FUSED 1) and with the sweep + stencil (0); the two give
    the same Hessenberg column and the same new reflector bit for bit."""
    legs = {f: _steps(oracle, N, hr.M, [(T_RIGHT_FUSED, f), (T_HH_FUSE, hh_fuse)], f"right fused={f} hh_fuse={hh_fuse}")[0]
            for f in (1, 0)}
    for (h1, p1), (h0, p0) in zip(legs[1], legs[0]):
        assert np.array_equal(h1, h0) and np.array_equal(p1, p0)


@pytest.mark.parametrize("hh_fuse", [1, 0])
def test_right_step_wonly_chains(oracle, hh_fuse):
    """The same at N = 130 on the w-only reflection chains (forced, two workgroups), where
    GK_TUNE_HH_FUSE 1 closes the step inside the UP chain and 0 launches the pieces: at the
    sizes above both values run the same launches."""
    N = hr.WONLY_SHAPE
    tunes = [(T_PC, -1), (T_RES, 1), (T_WONLY, 1), (T_R2, 12), (T_SHARE, 128), (T_TMO, 5000), (T_HH_FUSE, hh_fuse)]
    legs = {}
    for f in (1, 0):
        legs[f], plan = _steps(oracle, N, hr.M, tunes + [(T_RIGHT_FUSED, f)], f"right w-only fused={f} hh_fuse={hh_fuse}")
        assert plan["variant"] == "w-only", plan
    for (h1, p1), (h0, p0) in zip(legs[1], legs[0]):
        assert np.array_equal(h1, h0) and np.array_equal(p1, p0)


# ------------------------------------- 6. the one-launch update, bit for bit ----

@pytest.mark.parametrize("N", [2, 33, 64, 66, 130])
def test_right_update_one_launch_is_bit_identical(N):
    """x += M^-1 (P_1..P_m [y;0]) on planted reflectors, a seeded x and a seeded y: the cbpr2
    sweep with the accumulating output (GK_TUNE_RIGHT_FUSED 1) against the sweep into a work
    vector and k_add (0), np.array_equal, and one launch fewer under stencil + update.
    N = 2 and 33: tiny and odd (one point per lane); 64, 66: half a wave and a lane over it;
    130: two waves per line.  Then two cycles of the solve on either route: the same x."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    m = 3 if N == 2 else 6
    rng = np.random.default_rng(4200 + N)
    x0, y = rng.standard_normal(N * N), rng.standard_normal(m)
    got, launches = {}, {}
    for f in (1, 0):
        with _planted_right(N, m, [(T_RIGHT_FUSED, f)]) as c:
            c.set_x(x0)
            c.profile(True)
            c.profile_reset()
            nat.check(nat.hip().gk_hh_update_x(c.handle, y.ctypes.data_as(nat._dp), m), "gk_hh_update_x")
            prof = c.profile_read()
            c.profile(False)
            got[f] = c.get_x()
            launches[f] = prof["stencil"][1] + prof["update"][1]
    print(f"N={N}: stencil + update launches fused {launches[1]} two-launch {launches[0]}")
    assert np.all(np.isfinite(got[0])) and not np.array_equal(got[0], x0)
    assert np.array_equal(got[1], got[0])
    assert launches[0] == 2 and launches[1] == 1
    if N == 2:  # four unknowns: the Krylov space is exhausted inside the first cycle
        return
    sol = {}
    for f in (1, 0):
        with _right_ctx(N, m, fused=f) as c:
            sol[f] = ga.gmres_hh(c, tol=1e-15, precondition="right", max_cycles=2, want_hist=True)
    assert np.array_equal(sol[1].x, sol[0].x) and np.array_equal(sol[1].hist_res, sol[0].hist_res)


# --------------------------------------------------------------------- 7. slabs --

def _group_hh_right(N, m, nranks, max_cycles):
    """One host thread per rank over the in-process communicator (the set-up of
    test_gpu_right_precond.py section 7): local collectives only, no device exchange."""
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
            c.set_precond("cbpr2", PARAMS)
            c.set_rhs_ones()
            out[r] = ga.gmres_hh(c, tol=TOL, precondition="right", max_cycles=max_cycles, want_hist=True)
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
    """Two and three ranks (op_right's unfused route with halos, precond_sweeps + k_add for the
    update): the histories of the single-rank run."""
    N, m, cyc = 64, 10, 3
    ref = _hh_right_run(N, m, cyc, TOL)
    for nranks in (2, 3):
        res = _group_hh_right(N, m, nranks, cyc)
        assert len({(r.n_out, r.n_cycles) for r in res}) == 1
        assert np.array_equal(res[0].hist_res, res[-1].hist_res)
        print(f"{nranks} ranks: hist_res {res[0].hist_res.tolist()} single {ref.hist_res.tolist()}")
        assert len(res[0].hist_res) == len(ref.hist_res) == cyc
        assert np.allclose(res[0].hist_res, ref.hist_res, rtol=1e-5, atol=1e-13)


# ------------------------------------------------------------ 8. Fortran drop-in --

def test_right_fortran_dropin():
    """gmres_hh_prec_hip(..., side=GK_SIDE_RIGHT) through the reference's driver
    (`test_mfp_hip 64 10 hhright`: the Householder solve alone, tol 1e-15): the n_out, stages
    and final residual of the Python run of the same solve."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmres_amd", "lib",
                       "test_mfp_hip")
    out = subprocess.run([exe, "64", "10", "hhright"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "Householder Chebyshev on the right" in out.stdout and "MGSR" not in out.stdout
    line = lambda key: [l for l in out.stdout.splitlines() if key in l][0]  # noqa: E731
    its, stages = int(line("Iterations until convergence").split(":")[1].split()[0]), int(line("Stages=").split("Stages=")[1])
    ferr = float(line("Final residual, every digit").split(":")[1])
    r = _hh_right_run(64, 10, 1000, 1e-15)
    print(f"python: n_out {r.n_out} stages {r.cycles_out} final_err {r.final_err[r.n_out - 1]!r}; fortran: "
          f"iterations {its} stages {stages} final_err {ferr!r}")
    assert stages == r.cycles_out
    assert its - (stages - 1) * 10 == r.n_out
    assert np.isclose(ferr, r.final_err[r.n_out - 1], rtol=1e-5, atol=1e-13)
    assert ferr < 1e-15
    assert float(line("Max error L_max").split(":")[1]) < 1e-9
