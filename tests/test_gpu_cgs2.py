"""Solves with the opt-in CGS2 Arnoldi step (gk_set_orthogonalization GK_ORTH_CGS2): classical
Gram-Schmidt with one full reorthogonalisation -- batched dots, three reductions per step.

CGS2 is not bit-identical to the strict MGS-R step (gmres_mgsr.f90:341-360), so like the blocked
step it is held to the residual-history contract of tests/test_gpu_blocked.py (rtol 1e-5, atol
1e-13 per restart cycle; iterations to tol within +-1 %; ||x - 1||_inf < 1e-9) against the
reference's own runs (tests/golden/reference_runs.json) and the oracle, and the deviations are
printed (pytest -s).  tests/test_cgs2_data.py pins the same contract, and the orthogonality cap
used here, on a NumPy model without a GPU; the single step is checked against a long-double step
in tests/test_gpu_cgs2_step_known_answer.py.
"""
import ctypes
import json
import os
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "reference_runs.json")))
PARAMS = (8.2, 0.2)


def _dev(gpu, ref):
    g, r = np.asarray(gpu, dtype=float), np.asarray(ref, dtype=float)
    k = min(len(g), len(r))
    return float(np.max(np.abs(g[:k] - r[:k]) / np.abs(r[:k])))


def _contract(gpu, ref, rtol=1e-5, atol=1e-13):  # tests/test_gpu_blocked.py::_contract
    k = min(len(gpu), len(ref))
    assert k >= 1
    g, r = np.asarray(gpu[:k]), np.asarray(ref[:k])
    bad = np.abs(g - r) > rtol * np.abs(r) + atol
    assert not bad.any(), f"cycles {np.nonzero(bad)[0].tolist()} deviate: gpu={g} ref={r}"


def _run(N, m, cycles, orth="cgs2", tol=1e-15, want_x=False, want_verr=False, tunes=()):
    import gmres_amd as ga

    with ga.Context(N, m) as c:
        for k, v in tunes:
            c.tune(k, v)
        c.set_rhs_ones()
        c.set_orth(orth)
        plan = c.res_info()
        c.profile(True)
        c.profile_reset()
        r = ga.gmres_mgsr(c, tol, max_cycles=cycles, want_verr=want_verr, want_hist=True, want_x=want_x)
        return r, plan, c.profile_read()


_cache: dict = {}


def _run128(orth):
    """The 128^2, m = 30 solve to 1e-15 (and its first cycle's v_err); once per scheme."""
    if orth not in _cache:
        full = _run(128, 30, 1000, orth=orth, want_x=True)
        first = _run(128, 30, 1, orth=orth, want_verr=True)
        _cache[orth] = (full, first)
    return _cache[orth]


# ------------------------------------------------ against the reference's own runs ---

def test_cgs2_128_converges_like_reference():
    g = REF["mgsr_omp_identity_128_m30"]
    (r, plan, prof), _ = _run128("cgs2")
    assert plan["variant"] is None and prof["res"][1] == 0, (plan, prof)
    assert prof["graph"][1] >= r.iterations - 30, prof  # every step a replayed chain
    hi = [k for k, v in enumerate(g["hist_res"]) if v > 1e-10]
    print(f"\n[cgs2] 128^2: {r.iterations} iterations (reference {g['iterations']}), max rel dev "
          f"{_dev(r.hist_res[: len(hi)], g['hist_res'][: len(hi)]):.2e}, max |x - 1| {np.max(np.abs(r.x - 1.0)):.2e}")
    assert abs(r.iterations - g["iterations"]) <= 0.01 * g["iterations"]
    assert r.final_err[r.n_out - 1] < 1e-15
    assert np.max(np.abs(r.x - 1.0)) < 1e-9
    _contract(r.hist_res[: len(hi)], g["hist_res"][: len(hi)])


@pytest.mark.parametrize("key", ["mgsr_omp_identity_1024_m95_3cyc_t8", "mgsr_omp_identity_4096_m95_2cyc_t8"])
def test_cgs2_large_grids_vs_reference(key):
    g = REF[key]
    r, plan, prof = _run(g["N"], g["m"], g["max_cycles"])
    assert plan["variant"] is None and prof["res"][1] == 0, (plan, prof)
    assert r.n_cycles == g["max_cycles"]
    print(f"\n[cgs2] {key}: max rel dev vs reference {_dev(r.hist_res, g['hist_res']):.2e}")
    _contract(r.hist_res, g["hist_res"])


@pytest.mark.parametrize("N,m", [(127, 30), (100, 20), (96, 7)])
def test_cgs2_ragged_slabs_vs_oracle(oracle, N, m):
    """Odd n (the tail element), vectors that are no multiple of a workgroup's trip, small m
    (one ragged batch at every step): ten cycles against the oracle's gmres_mgsr_omp."""
    r, plan, _ = _run(N, m, 10)
    assert plan["variant"] is None
    ref = oracle.gmres_mgsr(oracle.rhs_ones(N), N, m, variant=oracle.MGSR_OMP, max_cycles=10)
    print(f"\n[cgs2] {N}^2 m={m}: max rel dev vs oracle {_dev(r.hist_res, ref.hist_res):.2e}")
    _contract(r.hist_res, ref.hist_res)


# -------------------------------------------------------- preconditioned solves ---

@pytest.mark.parametrize("N,m,kind,degree,side", [(64, 30, "cbpr2", 1, "right"), (48, 20, "cheb", 4, "left")])
def test_cgs2_preconditioned_solve_vs_mgsr(N, m, kind, degree, side):
    """To 1e-8 on one context: the CGS2 solve held to the same context's MGS-R solve; on the
    right final_err(n_out) is the true relative residual."""
    import gmres_amd as ga

    out = {}
    with ga.Context(N, m) as c:
        c.set_precond(kind, PARAMS, degree, side=side)
        c.set_rhs_ones()
        for orth in ("mgsr", "cgs2"):
            c.set_orth(orth)
            r = ga.gmres_mgsr(c, 1e-8, want_verr=False, want_hist=True)
            out[orth] = (r, c.true_residual())
    (rm, _), (rc, true_c) = out["mgsr"], out["cgs2"]
    print(f"\n[cgs2] {kind} {side} {N}^2 m={m}: {rc.iterations} iterations (MGS-R {rm.iterations}), max rel dev "
          f"{_dev(rc.hist_res, rm.hist_res):.2e}")
    assert rc.final_err[rc.n_out - 1] < 1e-8
    assert abs(rc.iterations - rm.iterations) <= max(1, 0.01 * rm.iterations)
    assert np.max(np.abs(rc.x - 1.0)) < 1e-6
    _contract(rc.hist_res, rm.hist_res)
    if side == "right":
        assert rc.final_err[rc.n_out - 1] == pytest.approx(true_c, rel=1e-6)


# ----------------------------------------------------------------- orthogonality ---

def test_cgs2_orthogonality_within_8x_of_mgsr():
    """gk_mgs_verr of the first 128^2 cycle: at most 8 x the MGS-R cycle's, the cap
    tests/test_cgs2_data.py pins on the NumPy model."""
    _, (rc, _, _) = _run128("cgs2")
    _, (rm, _, _) = _run128("mgsr")
    assert rc.n_out == rm.n_out == 30
    print(f"\n[cgs2] 128^2 first cycle v_err: CGS2 {rc.v_err[30]:.3e}, MGS-R {rm.v_err[30]:.3e}")
    assert 0.0 < rc.v_err[30] <= 8.0 * rm.v_err[30]


# --------------------------------------------------------------- row-block ranks ---

@pytest.mark.parametrize("R", [2, 4])
def test_cgs2_row_block_ranks(R):
    """R LocalGroup ranks at 256^2, m = 30, one cycle: the three all-reduces per step through
    the group's collectives; every rank takes the same decisions."""
    import gmres_amd as ga

    N, m = 256, 30
    single, _, _ = _run(N, m, 1)
    parts = ga.slab_partition(N, R)
    g = ga.LocalGroup(R)
    ctxs = [ga.Context(N, m, device=0, line0=l0, nlines=nl) for l0, nl in parts]
    out, err = [None] * R, []
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_local(g, r, max(nl for _, nl in parts))

        def work(q):
            try:
                c = ctxs[q]
                c.set_rhs_ones()
                c.set_orth("cgs2")
                c.profile(True)
                c.profile_reset()
                out[q] = (ga.gmres_mgsr(c, 1e-15, max_cycles=1, want_verr=False, want_hist=True), c.profile_read())
            except Exception as e:  # pragma: no cover - reported below
                err.append(e)

        th = [threading.Thread(target=work, args=(q,)) for q in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join(100)
        assert not err, err
        assert all(o is not None for o in out)
    finally:
        for c in ctxs:
            c.close()
        g.close()
    res = [o[0] for o in out]
    assert all(np.array_equal(res[0].hist_res, x.hist_res) for x in res)
    assert all(np.array_equal(res[0].final_err, x.final_err) for x in res)
    for _, prof in out:
        assert prof["res"][1] == 0 and 4 * m <= prof["proj"][1] <= 4 * m + 1, prof  # + the driver's one dot
    assert res[0].hist_res[0] == pytest.approx(single.hist_res[0], rel=1e-9)


# ------------------------------------------------------------ bit-identical runs ---

def test_cgs2_runs_are_bit_identical():
    """Two runs in a row, and the replayed graph against the chain call by call."""
    from gmres_amd import _native as nat

    a, _, pa = _run(100, 20, 5)
    b, _, _ = _run(100, 20, 5)
    c, _, pc = _run(100, 20, 5, tunes=[(nat.GK_TUNE_GRAPH, 0)])
    assert pa["graph"][1] > 0 and pc["graph"][1] == 0 and 4 * 100 <= pc["proj"][1] <= 4 * 100 + 5, (pa, pc)
    for o in (b, c):
        assert np.array_equal(a.hist_res, o.hist_res) and np.array_equal(a.hist_ferr, o.hist_ferr)


def test_mgsr_again_is_the_default_solve():
    """After set_orth("mgsr") the solve is a fresh context's default solve bit for bit, the
    resident plan back in res_info; the tuning values were kept meanwhile."""
    import gmres_amd as ga

    N, m = 256, 30
    with ga.Context(N, m) as c:
        c.set_rhs_ones()
        plan0, hh0 = c.res_info(), c.res_info(hh=True)
        c.set_orth("cgs2")
        assert c.orth == "cgs2" and c.res_info()["variant"] is None
        assert c.res_info(hh=True) == hh0 and hh0["variant"] is not None  # the Householder plan is unaffected
        mid = ga.gmres_mgsr(c, 1e-15, max_cycles=2, want_hist=True)
        c.set_precond("identity")  # kept across gk_set_precond / gk_set_precond_side
        assert c.orth == "cgs2"
        c.set_orth("mgsr")
        assert c.orth == "mgsr" and c.res_info() == plan0 and plan0["variant"] is not None
        back = ga.gmres_mgsr(c, 1e-15, max_cycles=3, want_hist=True)
    with ga.Context(N, m) as c:
        c.set_rhs_ones()
        fresh = ga.gmres_mgsr(c, 1e-15, max_cycles=3, want_hist=True)
    assert not np.array_equal(mid.hist_res, fresh.hist_res[:2])  # CGS2 did run in between
    assert np.array_equal(back.hist_res, fresh.hist_res) and np.array_equal(back.hist_ferr, fresh.hist_ferr)
    assert np.array_equal(back.x, fresh.x) and np.array_equal(back.v_err, fresh.v_err)


# ------------------------------------------------------------------ state errors ---

def test_cgs2_state_errors_and_unaffected_solvers():
    import gmres_amd as ga
    from gmres_amd import _native as nat

    L = nat.hip()
    hcol = np.zeros(12)
    hp = hcol.ctypes.data_as(nat._dp)
    v = ctypes.c_int(-1)

    def other_solves(c):
        c.set_precond("cbpr2", PARAMS)
        c.set_rhs_ones()
        hh = ga.gmres_hh(c, 1e-10, precondition=True, want_hist=True)
        x, it, res, hist = ga.pcg(c, tol=1e-9, max_iter=60, want_hist=True)
        return hh, x, it, hist

    with ga.Context(64, 10) as c:
        assert L.gk_get_orthogonalization(c.handle, ctypes.byref(v)) == nat.GK_OK and v.value == nat.GK_ORTH_MGSR
        assert L.gk_set_orthogonalization(c.handle, 2) == nat.GK_ERR_ARG
        assert L.gk_set_orthogonalization(c.handle, -1) == nat.GK_ERR_ARG
        assert c.orth == "mgsr"
        with pytest.raises(ValueError):
            c.set_orth("mgs")
        # FP32 columns are out of scope, either way round
        c.set_basis("f32")
        assert L.gk_set_orthogonalization(c.handle, nat.GK_ORTH_CGS2) == nat.GK_ERR_STATE
        c.set_basis("f64")
        hh_plan = c.res_info(hh=True)
        c.set_orth("cgs2")
        assert L.gk_set_basis_precision(c.handle, nat.GK_BASIS_F32) == nat.GK_ERR_STATE
        assert c.basis == "f64" and c.orth == "cgs2"
        assert c.res_info()["variant"] is None and c.res_info(hh=True) == hh_plan
        # a set inside an open cycle ends it
        c.set_rhs_ones()
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        assert L.gk_set_orthogonalization(c.handle, nat.GK_ORTH_CGS2) == nat.GK_OK  # the same value too
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        # the Householder cycle and the short-recurrence solvers do not ask the scheme
        hh_c, x_c, it_c, hist_c = other_solves(c)
    with ga.Context(64, 10) as c:
        hh_d, x_d, it_d, hist_d = other_solves(c)
    assert np.array_equal(hh_c.hist_res, hh_d.hist_res) and np.array_equal(hh_c.x, hh_d.x)
    assert it_c == it_d and np.array_equal(hist_c, hist_d) and np.array_equal(x_c, x_d)


# ---------------------------------------------------------------- Fortran drop-in ---

def test_cgs2_fortran_dropin():
    """gmres_mgsr_hip(..., orth=GK_ORTH_CGS2) through the reference's driver
    (`test_mfp_hip <N> <m> cgs2`: the MGS-R cycle alone, tol 1e-15)."""
    exe = os.path.join(os.path.dirname(HERE), "gmres_amd", "lib", "test_mfp_hip")
    out = subprocess.run([exe, "64", "20", "cgs2"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "CGS2 Chebyshev" in out.stdout and "Householder" not in out.stdout
    val = lambda key: float([l for l in out.stdout.splitlines() if key in l][0].split(":")[1].split()[0])  # noqa: E731
    max_cycles = 1000  # hip_max_restarts of gmres_hip.f90
    its = int([l for l in out.stdout.splitlines() if "Iterations until convergence" in l][0].split(":")[1].split()[0])
    assert val("Final residual") < 1e-15 * (1 + 1e-2) or its >= 20 * (max_cycles - 1)
    assert val("Max error L_max") < 1e-9
