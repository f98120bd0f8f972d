"""MGS-R GMRES(m) on an FP32-compressed Krylov basis (gk_set_basis_precision
GK_BASIS_F32) on the GPU: the columns are stored as FP32 and everything else stays FP64.

The stored values, the Hessenberg columns of a cycle and the solve histories are held
against the host restatement tests/cb_gmres_host.py; the resident step k_mgs_wcb against
the launch path of the same context; the driver's exit guard on the case that needs it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import verr_host
from tests.cb_gmres_host import CASES, GUARD_CASE, band, case_id, gmres_cb_host, host_solve

pytestmark = pytest.mark.gpu

PARAMS = (8.2, 0.2)
ULP32 = 2.0 ** -23


def _ctx(N, m, prec="identity", degree=8, side="left", basis="f32"):
    import gmres_amd as ga

    c = ga.Context(N, m)
    c.set_precond(prec, PARAMS, degree or 8, side=side)
    c.set_basis(basis)
    c.set_rhs_ones()
    return c


def _cycle(c, nsteps):
    """One cycle's first nsteps Arnoldi steps: the raw Hessenberg columns."""
    c.mgs_cycle_start()
    return [c.mgs_step(j) for j in range(1, nsteps + 1)]


def _roundtrip(v):
    return v.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------ 1. stored values ----

def test_cb_stored_values_are_float32():
    """Every column gk_get_basis returns equals its own float32 round trip; the same
    check on the FP64 basis finds a column that does not, so it can fail."""
    from gmres_amd import _native as nat

    N, m = 64, 6
    with _ctx(N, m) as c:
        assert c.basis == "f32"
        assert c.res_info()["variant"] == nat.RES_VARIANTS[nat.GK_RES_CB]
        _cycle(c, m)
        cols = [c.get_basis(k) for k in range(m + 1)]
    for k, v in enumerate(cols):
        assert np.all(np.isfinite(v)) and np.linalg.norm(v) > 0.5, k
        assert np.array_equal(v, _roundtrip(v)), k
    with _ctx(N, m, basis="f64") as c:
        assert c.basis == "f64"
        assert c.res_info()["variant"] != nat.RES_VARIANTS[nat.GK_RES_CB]
        _cycle(c, m)
        cols64 = [c.get_basis(k) for k in range(m + 1)]
    assert any(not np.array_equal(v, _roundtrip(v)) for v in cols64)


# ------------------------------------------- 2. cycle 1 against the restatement ----

_h1: dict = {}


def _host_cycle1(oracle, N, m, prec, side, threads=1):
    """Cycle 1 of the restatement (tol 1e-8, guarded, MGSR_MF control flow): the columns
    it forms before it leaves the cycle -- all m of them unless the Krylov space of a
    tiny grid is exhausted first (h < tol: the next column would be rounding noise over
    h) or the guard closes the cycle."""
    key = (N, m, prec, side, threads)
    if key not in _h1:
        _h1[key] = gmres_cb_host(oracle, N, m, prec=prec, side=side, tol=1e-8, max_cycles=1, threads=threads)
    return _h1[key]


@pytest.mark.parametrize("prec,side", [("identity", "left"), ("cbpr2", "right")])
@pytest.mark.parametrize("N", [2, 3, 5, 33, 64, 65, 130])
def test_cb_cycle1_matches_restatement(oracle, N, prec, side):
    """Each H(:,j) within 1e-9 ||H(:,j)|| of the restatement's: a factor 60 under 2^-24,
    which is what a column rounded differently, or not at all, shows, and far above FP64
    reordering (the restatement's own 1-vs-8-thread difference is printed beside it)."""
    m = max(3, min(8, N * N - 1))
    h = _host_cycle1(oracle, N, m, prec, side)
    h8 = _host_cycle1(oracle, N, m, prec, side, threads=8)
    ncol = h.n_outs[0]
    assert ncol == m or N <= 5, (ncol, m)
    with _ctx(N, m, prec, side=side) as c:
        cols = _cycle(c, ncol)
    for j in range(ncol):
        ref = h.H1[: j + 2, j]
        d = np.linalg.norm(cols[j] - ref) / np.linalg.norm(ref)
        d8 = np.linalg.norm(h8.H1[: j + 2, j] - ref) / np.linalg.norm(ref) if j < h8.n_outs[0] else float("nan")
        print(f"N={N} {prec}/{side} j={j + 1}: |H_dev - H_host| / |H| {d:.3e} (restatement 1 vs 8 threads {d8:.3e})")
        assert d <= 1e-9, (j + 1, d)


def test_cb_cycle1_control_f64_differs(oracle):
    """Control: the FP64 device solve is NOT within that bound of the FP32 restatement."""
    N, m = 64, 8
    for prec, side in (("identity", "left"), ("cbpr2", "right")):
        h = _host_cycle1(oracle, N, m, prec, side)
        with _ctx(N, m, prec, side=side, basis="f64") as c:
            cols = _cycle(c, m)
        d = [np.linalg.norm(cols[j] - h.H1[: j + 2, j]) / np.linalg.norm(h.H1[: j + 2, j]) for j in range(m)]
        print(f"{prec}/{side}: FP64 device vs FP32 restatement {['%.2e' % v for v in d]}")
        assert max(d) > 1e-9


# ------------------------------------------------ 3. every part of the kernel ----

def _all_parts_shape():
    """The smallest odd N whose slab on ONE workgroup (GK_TUNE_RES_SHARE 256 of 256 CUs)
    fills the register part, the LDS part, the streamed part and the odd tail element."""
    import gmres_amd as ga

    for N in range(257, 400, 2):
        p = ga.cb_plan_query(N * N, cus=256, share=256, m=4)
        if p["r2e"] == p["rw"] and p["l2e"] > 0 and p["nstream2"] > 0:
            return N
    raise AssertionError("no shape fills every part of k_mgs_wcb")


def _resident_vs_launch(N, share, m=4):
    from gmres_amd import _native as nat

    out = {}
    with _ctx(N, m) as c:
        c.tune(nat.GK_TUNE_RES_SHARE, share)
        for res in (1, 0):
            c.tune(nat.GK_TUNE_RES, res)
            info = c.res_info()
            cols = _cycle(c, m)
            out[res] = (info, cols, [c.get_basis(k) for k in range(m + 1)])
    return out


@pytest.mark.parametrize("shape", ["all-parts", (130, 1), (130, 16)], ids=str)
def test_cb_resident_step_against_launch_path(shape):
    """The H columns of the two routes of one context to the project's tolerance for two
    summation orders; the stored columns bit-identical, or at most 2 elements per
    column one FP32 ulp apart (a flip at a rounding boundary is legitimate)."""
    from gmres_amd import _native as nat

    N, share = (_all_parts_shape(), 256) if shape == "all-parts" else shape
    out = _resident_vs_launch(N, share)
    info = out[1][0]
    print(f"N={N} share={share}: resident plan {info}")
    assert info["variant"] == nat.RES_VARIANTS[nat.GK_RES_CB] and out[0][0]["variant"] is None
    if shape == "all-parts":
        assert info["G"] == 1 and info["r2e"] == info["r2"] and info["l2e"] > 0
        assert info["nres2"] < (N * N) // 2 and (N * N) % 2 == 1
    for a, b in zip(out[1][1], out[0][1]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-15)
    for k, (a, b) in enumerate(zip(out[1][2], out[0][2])):
        diff = np.flatnonzero(a != b)
        print(f"column {k}: {diff.size} elements differ between the routes")
        assert diff.size <= 2
        for e in diff:
            assert abs(a[e] - b[e]) <= ULP32 * max(abs(a[e]), abs(b[e])), (k, e, a[e], b[e])


# -------------------------------------------------- 4. launch path and graphs ----

def _solve(N, m, prec, degree, side, tol, cap, basis="f32", tunes=(), variant=None):
    import gmres_amd as ga

    with _ctx(N, m, prec, degree, side, basis) as c:
        for k, v in tunes:
            c.tune(k, v)
        r = ga.gmres_mgsr(c, tol=tol, variant=ga.MGSR_MF if variant is None else variant, max_cycles=cap,
                          want_hist=True)
        return r, c.true_residual()


def test_cb_launch_path_and_graphs():
    """GK_TUNE_RES 0 with the step graphs on and off: the same histories to rtol 1e-12,
    and both within 1e-6 relative of the resident run (the floor of test 5's band)."""
    from gmres_amd import _native as nat

    args = (64, 10, "cbpr2", 0, "left", 1e-15, 3)
    res, _ = _solve(*args)
    g1, _ = _solve(*args, tunes=[(nat.GK_TUNE_RES, 0), (nat.GK_TUNE_GRAPH, 1)])
    g0, _ = _solve(*args, tunes=[(nat.GK_TUNE_RES, 0), (nat.GK_TUNE_GRAPH, 0)])
    print(f"resident {res.hist_res.tolist()} graphs {g1.hist_res.tolist()} launches {g0.hist_res.tolist()}")
    assert res.n_cycles == g1.n_cycles == g0.n_cycles == 3
    assert np.allclose(g1.hist_res, g0.hist_res, rtol=1e-12, atol=0.0)
    assert np.allclose(g1.hist_ferr, g0.hist_ferr, rtol=1e-12, atol=1e-300)
    for r in (g1, g0):
        assert np.all(np.abs(r.hist_res - res.hist_res) <= 1e-6 * res.hist_res)


# ------------------------------------------------------------------ 5. histories ----

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cb_histories_match_restatement(oracle, case):
    """The device run against the guarded restatement: the same cycle count, n_out
    within one, hist_res[c] within max(1e-6, 100 S_c) relative (S_c: the restatement's
    own 1-vs-8-thread spread), and x: |x - 1| < 1e-5 where converged (host: <= 2.1e-6),
    the unconverged 130^2 case against the restatement's x to 1e-6."""
    N, m, prec, degree, side, tol, cap = case
    h = host_solve(oracle, case)
    S = band(oracle, case)
    r, _ = _solve(N, m, prec, degree, side, tol, cap)
    print(f"{case_id(case)}: cycles dev {r.n_cycles} host {h.n_cycles}, n_out dev {r.n_out} host {h.n_out}")
    assert r.n_cycles == h.n_cycles
    assert abs(r.n_out - h.n_out) <= 1
    k = min(len(S), r.n_cycles)
    rel = np.abs(r.hist_res[:k] - h.hist_res[:k]) / h.hist_res[:k]
    bound = np.maximum(1e-6, 100.0 * S[:k])
    print(f"{case_id(case)}: max rel dev of hist_res {rel.max():.3e} (bound there {bound[int(np.argmax(rel))]:.3e})")
    assert k == r.n_cycles and np.all(rel <= bound)
    converged = h.final_err[h.n_out - 1] < tol
    err = np.max(np.abs(r.x - (1.0 if converged else h.x)))
    print(f"{case_id(case)}: converged {converged}, max |x - {'1' if converged else 'x_host'}| {err:.3e}")
    assert err < (1e-5 if converged else 1e-6)


# ------------------------------------------------------------------ 6. the guard ----

def test_cb_exit_guard():
    """One cycle would take the estimate past what the basis resolves: the driver closes
    it at the floor (n_out 15 +- 1), the second cycle converges, and the exit estimate is
    the true residual."""
    N, m, prec, degree, side, tol, cap = GUARD_CASE
    r, true = _solve(N, m, prec, degree, side, tol, cap)
    n_out1 = int(np.count_nonzero(r.hist_ferr[0]))
    est = r.final_err[r.n_out - 1]
    print(f"cycles {r.n_cycles}, n_out {n_out1} then {r.n_out}, estimate {est:.3e}, true {true:.3e}")
    assert r.n_cycles == 2
    assert abs(n_out1 - 15) <= 1
    assert abs(est / true - 1.0) <= 1e-2
    assert true < tol


# ---------------------------------------------------------------------- 7. v_err ----

def test_cb_verr():
    """gk_mgs_verr on the float columns (the tree-reduced Gram) against the reference's
    formula evaluated on the columns gk_get_basis returns."""
    import gmres_amd as ga

    N, m = 64, 10
    with _ctx(N, m) as c:
        r = ga.gmres_mgsr(c, tol=1e-15, max_cycles=1)
        V = [c.get_basis(k) for k in range(m + 1)]
    assert r.n_out == m
    ref = verr_host.mgs_verr(V, m, verr_host.exact_dot)
    print(f"v_err dev {r.v_err[1:m + 1].tolist()} host {ref[1:m + 1].tolist()}")
    assert np.all(ref[1:m + 1] > 0.0)
    assert np.allclose(r.v_err[1:m + 1], ref[1:m + 1], rtol=1e-6, atol=0.0)


# ------------------------------------------------------- 8. state and rejections ----

def test_cb_rejections_and_switch_back():
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

    def pcg_hist(c):
        c.set_precond("cbpr2", PARAMS)
        c.set_rhs_ones()
        x, it, res, hist = ga.pcg(c, tol=1e-9, max_iter=60, want_hist=True)
        return x, it, hist

    with ga.Context(64, 2) as c:  # the two widened vectors need m >= 3
        assert L.gk_set_basis_precision(c.handle, nat.GK_BASIS_F32) == nat.GK_ERR_ARG
        assert c.basis == "f64"
    N = 64
    g = ga.LocalGroup(2)
    parts = ga.slab_partition(N, 2)
    ranks = [ga.Context(N, 10, line0=l0, nlines=nl) for l0, nl in parts]
    try:
        for r, c in enumerate(ranks):
            c.comm_init_local(g, r, max(nl for _, nl in parts))
        assert L.gk_set_basis_precision(ranks[0].handle, nat.GK_BASIS_F32) == nat.GK_ERR_STATE
        assert "single-rank" in nat.last_error()
    finally:
        for c in ranks:
            c.close()
        g.close()
    with ga.Context(N, 10) as c:
        assert L.gk_set_basis_precision(c.handle, 2) == nat.GK_ERR_ARG
        c.set_basis("f32")
        g1 = ga.LocalGroup(1)
        try:
            assert L.gk_comm_init_local(c.handle, g1.handle, 0, N) == nat.GK_ERR_STATE
            assert "single-rank" in nat.last_error()
        finally:
            g1.close()
        c.set_precond("cbpr2", PARAMS)
        c.set_rhs_ones()
        # Householder GMRES does not run on the compressed basis
        assert L.gk_hh_cycle_start(c.handle, 1, ctypes.byref(d)) == nat.GK_ERR_STATE
        assert "MGS-R only" in nat.last_error()
        # setting the precision ends the open cycle
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        assert L.gk_set_basis_precision(c.handle, nat.GK_BASIS_F64) == nat.GK_OK
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        c.mgs_cycle_start()
        assert L.gk_mgs_step(c.handle, 1, hp) == nat.GK_OK
        assert L.gk_set_basis_precision(c.handle, nat.GK_BASIS_F32) == nat.GK_OK
        assert L.gk_mgs_step(c.handle, 2, hp) == nat.GK_ERR_STATE
        # the short-recurrence solvers own their columns as FP64
        assert c.basis == "f32"
        x32, it32, hist32 = pcg_hist(c)
        # back on FP64: a default solve is the one of a fresh context, bit for bit
        c.set_basis("f64")
        back = default_solve(c)
    with ga.Context(N, 10) as c:
        x64, it64, hist64 = pcg_hist(c)
        fresh = default_solve(c)
    assert it32 == it64 and np.array_equal(hist32, hist64) and np.array_equal(x32, x64)
    assert np.array_equal(back.hist_res, fresh.hist_res)
    assert np.array_equal(back.hist_ferr, fresh.hist_ferr)
    assert np.array_equal(back.x, fresh.x)
    assert np.array_equal(back.v_err, fresh.v_err)


# ------------------------------------------------------------ 9. Fortran drop-in ----

def test_cb_fortran_dropin():
    """gmres_mgsr_hip(..., basis=GK_BASIS_F32) through the reference's driver
    (`test_mfp_hip <N> <m> f32`: the MGS-R solve alone, tol 1e-15).  The solve ends below
    tol, or -- the estimate hovering at rounding level -- at the driver's cap of
    restarts; either way the solution is x = 1."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmres_amd", "lib",
                       "test_mfp_hip")
    out = subprocess.run([exe, "48", "20", "f32"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "compressed basis" in out.stdout and "Householder" not in out.stdout
    val = lambda key: float([l for l in out.stdout.splitlines() if key in l][0].split(":")[1].split()[0])  # noqa: E731
    max_cycles = 1000  # hip_max_restarts of gmres_hip.f90
    its = int([l for l in out.stdout.splitlines() if "Iterations until convergence" in l][0].split(":")[1].split()[0])
    assert val("Final residual") < 1e-15 * (1 + 1e-2) or its >= 20 * (max_cycles - 1)
    assert val("Max error L_max") < 1e-9
