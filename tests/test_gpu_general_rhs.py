"""Solves from a right-hand side without the square's symmetries, through Context.set_rhs(b)
(tests/general_data.general_rhs: b = A x_true, x_true seeded Gaussian).

Every other solve-level GPU test uses b = A*1, which the eight symmetries of the square leave
invariant -- and with it every Krylov vector and iterate, so a kernel that reads element
n-1-k for k, walks a tail from the wrong end or swaps the ends of a slab reproduces those
histories bit for bit, and |x - 1| cannot see a permuted x.  Here every kernel family is
pinned to an independent computation on asymmetric data: the CPU oracle (MGS-R, Householder,
PCG, BiCGSTAB), the host restatements (right preconditioning, the FP32 basis), and the
single-context run (slabs).

Per-cycle true residuals keep the rule of each variant's sibling test (named at the helper),
and no bound drops below 10 x the reference's own deviation between 1 and 7 threads on the
same case, computed at run time from the reference alone: on general b the oracle's own
spread comes close to the old rule at N = 256.  The solution is held to the oracle's x,
max |x - x_oracle| <= 1e-9 max |x_true|, and gk_true_residual to the last history entry.
"""
import threading

import numpy as np
import pytest

from tests.general_data import general_rhs

pytestmark = pytest.mark.gpu

PARAMS = (8.2, 0.2)
T_RES, T_R2, T_SHARE, T_TMO, T_WONLY, T_HH_FUSE, T_PC, T_BLOCK, T_XTMO = 8, 9, 10, 11, 13, 15, 21, 23, 7

_rhs: dict = {}
_orc: dict = {}
_dev: dict = {}


def _gen(oracle, N):
    """(x_true, b) of the N x N grid, once per N; callers do not modify them."""
    if N not in _rhs:
        _rhs[N] = general_rhs(oracle, N, 900 + N)
    return _rhs[N]


def _kind(oracle, prec):
    return {"identity": oracle.PREC_IDENTITY, "cbpr2": oracle.PREC_CBPR2, "cheb": oracle.PREC_CHEB}[prec]


def _oracle(oracle, method, N, m, prec, degree, cycles):
    """(the oracle's run at one thread, |hist_res(1 thread) - hist_res(7 threads)| per cycle),
    once per case."""
    key = (method, N, m, prec, degree, cycles)
    if key not in _orc:
        _, b = _gen(oracle, N)

        def run(th):
            if method == "mgsr":
                return oracle.gmres_mgsr(b, N, m, prec=_kind(oracle, prec), params=PARAMS, degree=degree,
                                         variant=oracle.MGSR_OMP, max_cycles=cycles, threads=th)
            return oracle.gmres_hh(b, N, m, prec=_kind(oracle, prec), params=PARAMS, degree=degree,
                                   midcycle_exit=int(prec != "identity"), max_cycles=cycles, threads=th)

        r1, r7 = run(1), run(7)
        assert len(r1.hist_res) == len(r7.hist_res) == cycles
        _orc[key] = (r1, np.abs(r1.hist_res - r7.hist_res))
    return _orc[key]


def _res_tunes(r2, share, wonly, pc):
    return [(T_PC, pc), (T_RES, 1), (T_WONLY, wonly), (T_R2, r2), (T_SHARE, share), (T_TMO, 5000)]


def _solve(N, m, prec, degree, tunes, b, method="mgsr", cycles=4, side="left", tol=1e-15, variant=None,
           basis=None, keep_basis=0):
    """One device solve from set_rhs(b): (result, gk_true_residual afterwards, the step's plan,
    profile, basis columns if asked for)."""
    import gmres_amd as ga

    with ga.Context(N, m) as c:
        for k, v in tunes:
            c.tune(k, v)
        c.set_precond(prec, PARAMS, degree, side=side)
        if basis is not None:
            c.set_basis(basis)
        c.set_rhs(b)
        c.profile(True)
        c.profile_reset()
        if method == "mgsr":
            r = ga.gmres_mgsr(c, tol, variant=ga.MGSR_OMP if variant is None else variant, max_cycles=cycles,
                              want_hist=True)
        else:
            r = ga.gmres_hh(c, tol, precondition=(prec != "identity"), max_cycles=cycles, want_hist=True)
        prof = c.profile_read()
        c.profile(False)
        true = c.true_residual()
        plan = c.res_info(hh=method == "hh")
        cols = None
        if keep_basis:
            cols = ([c.get_basis(k, 0) for k in range(keep_basis)],
                    [c.get_basis(k, 1) for k in range(keep_basis)] if method == "hh" else None)
    return r, true, plan, prof, cols


def _launch_run(oracle, method, N, m, prec, degree, cycles):
    """The launch-path run of a case (GK_TUNE_RES 0), once per case."""
    key = (method, N, m, prec, degree, cycles)
    if key not in _dev:
        _dev[key] = _solve(N, m, prec, degree, [(T_RES, 0)], _gen(oracle, N)[1], method=method, cycles=cycles)
    return _dev[key]


def _mgsr_pair(r):  # test_gpu_resident.py::test_resident_matches_launch_path
    return np.where(r > 1e-8, 1e-10, 1e-4)


def _hh_pair(r):  # test_gpu_resident.py::test_resident_householder_matches_launch_path
    return np.where(r > 1e-6, 1e-9, np.where(r > 1e-12, 1e-3, 5e-2))


def _hh_fuse_pair(r):  # test_gpu_resident.py::test_householder_fused_step_matches_unfused
    return np.where(r > 1e-6, 1e-10, np.where(r > 1e-12, 1e-4, 5e-2))


def _hh_oracle(r):  # test_gpu_solver.py::_hist_close_hh
    return np.where(r > 1e-6, 1e-8, np.where(r > 1e-12, 1e-3, 5e-2))


def _hist(h, r, bound, spread, what):
    """|h - r| <= max(bound, 10 x the reference's own 1-vs-7-thread spread), per cycle."""
    h, r = np.asarray(h), np.asarray(r)
    assert len(h) == len(r), (what, len(h), len(r))
    lim = np.maximum(bound, 10.0 * spread)
    dev = np.abs(h - r)
    print(f"{what}: residuals {h.tolist()}; worst dev/bound {np.max(dev / lim):.3e}; oracle 1-vs-7-thread spread "
          f"over the rule's bound {np.max(spread / bound):.3e}")
    assert np.all(dev <= lim), (what, h, r, lim)


def _solution(r, true, x_ref, x_true, what):
    err = np.max(np.abs(r.x - x_ref))
    print(f"{what}: max |x - x_ref| {err:.3e} (bound {1e-9 * np.max(np.abs(x_true)):.3e}); true residual {true!r}, "
          f"last history entry {r.hist_res[-1]!r}")
    assert err <= 1e-9 * np.max(np.abs(x_true)), what
    assert abs(true - r.hist_res[-1]) <= 1e-12 * r.hist_res[-1], what


# ------------------------------------------------------------------------ MGS-R ---

# (route, N, m, tuning, res_info variant): the launch path on every shape; one forcing per
# resident family at the shapes where its plan applies (N = 45 is always the prefetch kernel);
# the blocked step S = 2
MGSR_ROUTES = [
    ("launch", 45, 12, [(T_RES, 0)], None), ("launch", 130, 30, [(T_RES, 0)], None),
    ("launch", 256, 40, [(T_RES, 0)], None),
    ("prefetch", 45, 12, _res_tunes(2, 64, -1, -1), "prefetch"),       # odd N, 2 workgroups
    ("prefetch", 130, 30, _res_tunes(2, 8, -1, -1), "prefetch"),       # streamed tail
    ("prefetch", 256, 40, _res_tunes(12, 16, -1, -1), "prefetch"),     # R2 = 8
    ("pairs", 130, 30, _res_tunes(0, 128, 0, 0), "pairs"),
    ("pairs+lds", 256, 40, _res_tunes(0, 64, 0, 0), "pairs+lds"),
    ("w-only", 130, 30, _res_tunes(0, 128, 1, 0), "w-only"),
    ("w-only", 256, 40, _res_tunes(0, 64, 1, 0), "w-only"),
    ("w+column", 130, 30, _res_tunes(0, 128, -1, 1), "w+column"),
    ("w+column", 256, 40, _res_tunes(0, 64, -1, 1), "w+column"),
    ("blocked2", 45, 12, [(T_BLOCK, 2), (T_TMO, 10000)], "blocked"),
    ("blocked2", 130, 30, [(T_BLOCK, 2), (T_TMO, 10000)], "blocked"),
    ("blocked2", 256, 40, [(T_BLOCK, 2), (T_TMO, 10000)], "blocked"),
]


@pytest.mark.parametrize("prec,degree", [("identity", 1), ("cbpr2", 1), ("cheb", 4)])
@pytest.mark.parametrize("route,N,m,tunes,variant", MGSR_ROUTES, ids=[f"{r[0]}-{r[1]}" for r in MGSR_ROUTES])
def test_mgsr_general_rhs(oracle, route, N, m, tunes, variant, prec, degree):
    """Four cycles of MGS-R against the oracle (1e-5 r + 1e-13, test_gpu_resident.py::
    test_resident_vs_oracle_to_convergence) and, for the strict resident kernels, against the
    launch path (1e-10 r above 1e-8, 1e-4 r below); x against the oracle's x."""
    x_true, b = _gen(oracle, N)
    ref, spread = _oracle(oracle, "mgsr", N, m, prec, degree, 4)
    if route == "launch":
        r, true, plan, prof, _ = _launch_run(oracle, "mgsr", N, m, prec, degree, 4)
    else:
        r, true, plan, prof, _ = _solve(N, m, prec, degree, tunes, b)
    what = f"mgsr {route} N={N} m={m} {prec}"
    print(f"{what}: plan {plan}")
    assert plan["variant"] == variant, plan
    if variant is None:
        assert prof["res"][1] == 0 and prof["proj"][1] + prof["graph"][1] > 0, prof
    else:  # the resident kernel ran every step (k_proj only in the off-cycle diagnostics)
        assert prof["res"][1] >= 4 * m and prof["proj"][1] < prof["res"][1] // 4, prof
    assert r.n_cycles == 4
    _hist(r.hist_res, ref.hist_res, 1e-5 * ref.hist_res + 1e-13, spread, what + " vs oracle")
    if variant not in (None, "blocked"):
        lr = _launch_run(oracle, "mgsr", N, m, prec, degree, 4)[0]
        _hist(r.hist_res, lr.hist_res, _mgsr_pair(lr.hist_res) * lr.hist_res + 1e-16, spread, what + " vs launch path")
    _solution(r, true, ref.x, x_true, what)


# ------------------------------------------------------------------ Householder ---

def _hh_cycles(N):
    return 4 if N <= 256 else 2  # the oracle at N = 300 / 512 stays near a second


def _hh_cases():
    from tests import test_gpu_resident as tr

    out = [("launch", 64, 20, "identity", [(T_RES, 0)], None), ("launch", 45, 12, "cbpr2", [(T_RES, 0)], None),
           ("launch", 256, 40, "identity", [(T_RES, 0)], None)]
    for N, m, prec, r2, share, wonly in tr.HCASES:
        fuses = (1, 0) if wonly == 1 else (1,)
        for f in fuses:
            out.append((f"res-fuse{f}", N, m, prec, _res_tunes(r2, share, wonly, -1) + [(T_HH_FUSE, f)],
                        "w-only" if wonly == 1 else "any"))
    for N, m, prec, r2, share, wonly in tr.HPCASES:
        out.append(("res-pc", N, m, prec, _res_tunes(r2, share, wonly, 1), "w+column"))
    return out


HH_CASES = _hh_cases()


@pytest.mark.parametrize("route,N,m,prec,tunes,variant", HH_CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in HH_CASES])
def test_householder_general_rhs(oracle, route, N, m, prec, tunes, variant):
    """gmres_hh (identity: full cycles; cbpr2: precondition = True) on the launch path and as
    resident reflection chains (the HCASES / HPCASES forcing of test_gpu_resident.py, the
    w-only chains with GK_TUNE_HH_FUSE 1 and 0): against the oracle with the Householder
    tiers of test_gpu_solver.py, against the launch path with those of test_gpu_resident.py."""
    x_true, b = _gen(oracle, N)
    cyc = _hh_cycles(N)
    ref, spread = _oracle(oracle, "hh", N, m, prec, 8, cyc)
    what = f"hh {route} N={N} m={m} {prec}"
    if route == "launch":
        r, true, plan, prof, _ = _launch_run(oracle, "hh", N, m, prec, 8, cyc)
        assert plan["variant"] is None and prof["res"][1] == 0, (plan, prof)
    else:
        r, true, plan, prof, _ = _solve(N, m, prec, 8, tunes, b, method="hh", cycles=cyc)
        print(f"{what}: plan {plan}")
        assert plan["variant"] is not None and (variant == "any" or plan["variant"] == variant), plan
        assert prof["res"][1] > 0 and prof["proj"][1] < prof["res"][1] // 4, prof  # k_proj: diagnostics only
    assert r.n_cycles == cyc
    _hist(r.hist_res, ref.hist_res, _hh_oracle(ref.hist_res) * ref.hist_res + 1e-16, spread, what + " vs oracle")
    if route != "launch":
        lr = _launch_run(oracle, "hh", N, m, prec, 8, cyc)[0]
        _hist(r.hist_res, lr.hist_res, _hh_pair(lr.hist_res) * lr.hist_res + 1e-16, spread, what + " vs launch path")
    if route == "res-fuse0":  # the fused and the unfused step of the same chains
        fr = _solve(N, m, prec, 8, tunes[:-1] + [(T_HH_FUSE, 1)], b, method="hh", cycles=cyc)[0]
        _hist(r.hist_res, fr.hist_res, _hh_fuse_pair(fr.hist_res) * fr.hist_res + 1e-16, spread, what + " vs fused")
    _solution(r, true, ref.x, x_true, what)


@pytest.mark.parametrize("N,m,prec", [(64, 20, "identity"), (45, 12, "cbpr2")])
def test_hh_verr_by_value_general_rhs(oracle, N, m, prec):
    """gk_hh_verr on the reflectors of a general-b solve: the rebuilt basis and the diagnostic
    equal the reference's formula evaluated on the device reflectors, bit for bit
    (test_gpu_solver.py::test_hh_verr_by_value)."""
    from tests import verr_host as vh

    r, _, _, _, (P, Vb) = _solve(N, m, prec, 8, [], _gen(oracle, N)[1], method="hh", cycles=2, keep_basis=m)
    n = r.n_out
    assert n == m
    dot = vh.ref_dot(oracle)
    Vh = vh.hh_rebuild(P, n, dot)
    assert all(np.array_equal(a, b) for a, b in zip(Vb, Vh))
    assert np.array_equal(r.v_err[1:n], vh.hh_verr_of_basis(Vh, n, dot)[1:n])
    assert np.all(r.v_err[1:n] >= 0.0) and np.any(r.v_err[1:n] > 0.0)


# ------------------------------------------------------------------- right side ---

RIGHT = [("cbpr2-fused", "cbpr2", 1, 1), ("cbpr2-two-launch", "cbpr2", 1, 0), ("cheb3", "cheb", 3, 1)]


@pytest.mark.parametrize("N,m", [(65, 16), (130, 12)])
@pytest.mark.parametrize("kind,prec,degree,fused", RIGHT, ids=[k[0] for k in RIGHT])
def test_right_side_general_rhs(oracle, kind, prec, degree, fused, N, m):
    """Three cycles on the right against tests/right_gmres_host.py with the same b (rtol 1e-5,
    atol 1e-13: test_gpu_right_precond.py::test_right_histories_match_host), and final_err at
    the end of every cycle is the true residual: a decade over the host's own gap, floor 1e-9
    (test_right_estimate_is_the_true_residual)."""
    import gmres_amd as ga
    from gmres_amd import _native as nat
    from tests.right_gmres_host import gmres_mgsr_host

    x_true, b = _gen(oracle, N)
    cyc = 3
    key = ("right", N, m, prec, degree)
    if key not in _orc:
        h1, h7 = (gmres_mgsr_host(oracle, N, m, prec=prec, degree=degree, side="right", tol=1e-15, max_cycles=cyc,
                                  b=b, threads=th) for th in (1, 7))
        _orc[key] = (h1, np.abs(h1.hist_res - h7.hist_res))
    h, spread = _orc[key]
    r, true, _, _, _ = _solve(N, m, prec, degree, [(nat.GK_TUNE_RIGHT_FUSED, fused)], b, cycles=cyc, side="right",
                              variant=ga.MGSR_MF)
    what = f"right {kind} N={N}"
    assert r.n_cycles == h.n_cycles == cyc and r.n_out == h.n_out == m
    _hist(r.hist_res, h.hist_res, 1e-5 * h.hist_res + 1e-13, spread, what + " vs host")
    assert np.allclose(r.hist_ferr, h.hist_ferr, rtol=1e-5, atol=1e-13)
    gap_dev = max(abs(r.hist_ferr[c, m - 1] / r.hist_res[c] - 1.0) for c in range(cyc))
    print(f"{what}: gap_dev {gap_dev:.3e} gap_host {h.gap():.3e}")
    assert gap_dev <= max(10.0 * h.gap(), 1e-9)
    _solution(r, true, h.x, x_true, what)


# ------------------------------------------------------------------- FP32 basis ---

@pytest.mark.parametrize("route", ["resident", "launch"])
@pytest.mark.parametrize("prec,side", [("identity", "left"), ("cbpr2", "right")])
@pytest.mark.parametrize("N,m", [(33, 8), (130, 12)])
def test_fp32_basis_general_rhs(oracle, N, m, prec, side, route):
    """The compressed basis against tests/cb_gmres_host.py with the same b: the same cycle
    count, n_out within one, hist_res within max(1e-6, 100 S_c) relative, S_c the
    restatement's own 1-vs-8-thread spread (test_gpu_cb.py::test_cb_histories_match_restatement);
    every stored column equals its own float32 round trip."""
    import gmres_amd as ga
    from gmres_amd import _native as nat
    from tests.cb_gmres_host import gmres_cb_host

    x_true, b = _gen(oracle, N)
    tol, cap = 1e-8, 4
    key = ("cb", N, m, prec, side)
    if key not in _orc:
        _orc[key] = tuple(gmres_cb_host(oracle, N, m, prec=prec, side=side, tol=tol, max_cycles=cap, threads=th, b=b)
                          for th in (1, 8))
    h, h8 = _orc[key]
    k8 = min(h.n_cycles, h8.n_cycles)
    S = np.maximum.accumulate(np.abs(h8.hist_res[:k8] - h.hist_res[:k8]) / h.hist_res[:k8])
    tunes = [] if route == "resident" else [(T_RES, 0)]
    r, true, plan, _, (cols, _) = _solve(N, m, prec, 8, tunes, b, cycles=cap, side=side, tol=tol, variant=ga.MGSR_MF,
                                         basis="f32", keep_basis=m + 1)
    what = f"fp32 basis {route} N={N} {prec}/{side}"
    assert plan["variant"] == (nat.RES_VARIANTS[nat.GK_RES_CB] if route == "resident" else None), plan
    print(f"{what}: cycles dev {r.n_cycles} host {h.n_cycles}, n_out dev {r.n_out} host {h.n_out}")
    assert r.n_cycles == h.n_cycles and abs(r.n_out - h.n_out) <= 1
    k = min(len(S), r.n_cycles)
    rel = np.abs(r.hist_res[:k] - h.hist_res[:k]) / h.hist_res[:k]
    bound = np.maximum(1e-6, 100.0 * S[:k])
    print(f"{what}: max rel dev of hist_res {rel.max():.3e} (bound there {bound[int(np.argmax(rel))]:.3e})")
    assert k == r.n_cycles and np.all(rel <= bound)
    for i, v in enumerate(cols):
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), i
    assert any(np.linalg.norm(v) > 0.5 for v in cols)
    converged = h.final_err[h.n_out - 1] < tol
    err = np.max(np.abs(r.x - (x_true if converged else h.x))) / np.max(np.abs(x_true))
    print(f"{what}: converged {converged}, max |x - {'x_true' if converged else 'x_host'}| / max |x_true| {err:.3e}")
    assert err < (1e-5 if converged else 1e-6)
    assert abs(true - r.hist_res[-1]) <= 1e-12 * r.hist_res[-1]


# ------------------------------------------------------------ short recurrences ---

@pytest.mark.parametrize("N,blocks", [(63, 0), (63, 7), (96, 0), (96, 7), (129, 0), (129, 7)])
@pytest.mark.parametrize("prec", ["identity", "cbpr2", "cheb"])
@pytest.mark.parametrize("solver", ["pcg", "pbicgstab"])
def test_short_recurrence_general_rhs(oracle, solver, prec, N, blocks):
    """The fused passes (line marches; with cbpr2 the two-level marches) from a general b:
    against the operation sequence on the same device (the assertions of test_gpu_sr.py::
    test_fused_matches_operation_sequence), against the oracle over the first decade
    (_close_early), GK_TUNE_SR_TWO_LEVEL 1 against 0 bit for bit, and x against x_true."""
    import gmres_amd as ga
    from gmres_amd import _native as nat
    from tests.test_gpu_sr import _close_early

    x_true, b = _gen(oracle, N)
    tol = 1e-9
    key = (solver, N, prec)
    if key not in _orc:
        _orc[key] = getattr(oracle, solver)(b, N, tol, 4000, _kind(oracle, prec), params=PARAMS, degree=4)
    _, ref_it, ref_res, ref_hist = _orc[key]
    out = {}
    for two in (1, 0):
        with ga.Context(N, 8) as c:
            c.tune(nat.GK_TUNE_SR_TWO_LEVEL, two)
            if blocks:
                c.tune(nat.GK_TUNE_SR_BLOCKS, blocks)
            c.set_precond(prec, PARAMS, 4)
            c.set_rhs(b)
            out[two] = getattr(ga, solver)(c, tol, 4000, want_hist=True, fused=True)
            if two:
                seq = getattr(ga, solver)(c, tol, 4000, want_hist=True, fused=False)
    (xf, itf, rf, hf), (x0, it0, r0, h0), (xs, its, rs, hs) = out[1], out[0], seq
    assert itf == it0 and np.array_equal(hf, h0) and np.array_equal(xf, x0)
    assert rf < tol and rs < tol and ref_res < tol
    assert len(hf) == itf and len(hs) == its and hf[-1] == rf
    if solver == "pcg":
        assert abs(itf - its) <= 2, (itf, its)
        assert abs(itf - ref_it) <= max(2, 0.03 * ref_it), (itf, ref_it)
        k = min(len(hf), len(hs))
        dev = np.abs(hf[:k] - hs[:k]) / hs[:k]
        assert np.all(dev[hs[:k] > 1e-4 * hs[0]] <= 1e-9), dev.max()
    else:
        assert abs(itf - its) <= max(3, 0.15 * its), (itf, its)
        assert abs(itf - ref_it) <= max(3, 0.15 * ref_it), (itf, ref_it)
        assert _close_early(hf, hs, 1e-9) <= 1e-9
    early = _close_early(hf, ref_hist, 1e-9)
    errs = [np.max(np.abs(x - x_true)) / np.max(np.abs(x_true)) for x in (xf, xs)]
    print(f"{solver} {prec} N={N} blocks={blocks}: {itf} iterations (sequence {its}, oracle {ref_it}); first decade vs "
          f"oracle {early:.3e}; max |x - x_true| / max |x_true| fused {errs[0]:.3e} sequence {errs[1]:.3e}")
    assert early <= 1e-9
    assert max(errs) <= 1e-6


# ------------------------------------------------------------------------ slabs ---

def _splits(N):
    import gmres_amd as ga

    w = (N - 4) // 2  # a slab of exactly the Chebyshev degree's 4 lines between wide ones
    return {"even2": ga.slab_partition(N, 2), "even3": ga.slab_partition(N, 3), "thin": [(0, w), (w, 4), (w + 4, N - w - 4)]}


def _slab_solve(c, method, prec):
    import gmres_amd as ga

    if method == "mgsr":
        return ga.gmres_mgsr(c, 1e-15, max_cycles=2, want_hist=True)
    if method == "hh":
        return ga.gmres_hh(c, 1e-15, precondition=(prec != "identity"), max_cycles=2, want_hist=True)
    x, it, res, hist = ga.pcg(c, 0.0, 25, want_hist=True)  # a fixed 25 iterations
    return x, hist


def _slab_run(N, m, parts, transport, method, prec, degree, b):
    import gmres_amd as ga

    R = len(parts)
    g = ga.LocalGroup(R)
    ctxs = [ga.Context(N, m, device=0, line0=l0, nlines=nl) for l0, nl in parts]
    out, err = [None] * R, []
    try:
        for q, c in enumerate(ctxs):
            c.comm_init_local(g, q, max(nl for _, nl in parts))
        if transport != "local":
            for c in ctxs:
                c.xchg_local()
                c.tune(T_XTMO, 5000)
                if transport == "xchg-res":
                    c.tune(T_RES, 1)
                    c.tune(T_TMO, 5000)

        def work(q):
            try:
                c = ctxs[q]
                l0, nl = parts[q]
                c.set_precond(prec, PARAMS, degree)
                c.set_rhs(b[l0 * N:(l0 + nl) * N])
                c.profile(True)
                c.profile_reset()
                out[q] = (_slab_solve(c, method, prec), c.profile_read())
            except Exception as e:  # pragma: no cover - reported below
                err.append(e)

        th = [threading.Thread(target=work, args=(q,)) for q in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        assert not err, err
        assert all(o is not None for o in out)
    finally:
        for c in ctxs:
            c.close()
        g.close()
    return out


SLAB_METHODS = [("mgsr", "identity", 1), ("mgsr", "cheb", 4), ("hh", "identity", 1), ("pcg", "cbpr2", 1)]
# (the short-recurrence passes have no resident launch: no xchg-res case for PCG)
SLAB_CASES = [(me, pr, dg, sp, tr) for me, pr, dg in SLAB_METHODS for sp in ("even2", "even3", "thin")
              for tr in ("local", "xchg", "xchg-res") if not (me == "pcg" and tr == "xchg-res")]


@pytest.mark.parametrize("method,prec,degree,split,transport", SLAB_CASES, ids=["-".join(map(str, s)) for s in SLAB_CASES])
def test_slabs_general_rhs(oracle, method, prec, degree, split, transport):
    """N = 130 as 2 and 3 LocalGroup ranks on one GPU (and the uneven 63 / 4 / 63 split), each
    rank given its slab of b, over the in-process group, the device exchange, and the device
    exchange with resident launches: every rank takes the same decisions, the history follows
    the single-context run within the tiers of test_gpu_xgmi.py::_check_against_single (PCG:
    test_gpu_sr.py::test_slabs_match_single_context), and the concatenated x is the
    single-context x to 1e-12 relative."""
    import gmres_amd as ga

    N, m = 130, 12
    x_true, b = _gen(oracle, N)
    key = ("single", method, prec)
    if key not in _dev:
        with ga.Context(N, m) as c:
            c.set_precond(prec, PARAMS, degree)
            c.set_rhs(b)
            _dev[key] = _slab_solve(c, method, prec)
    single = _dev[key]
    out = _slab_run(N, m, _splits(N)[split], transport, method, prec, degree, b)
    res = [o[0] for o in out]
    what = f"slabs {method} {prec} {split} {transport}"
    if transport == "xchg-res":
        assert all(o[1]["res"][1] > 0 for o in out), [o[1] for o in out]
    if method == "pcg":
        h0, xs = single[1], single[0]
        assert all(np.array_equal(res[0][1], h) for _, h in res)
        h = res[0][1]
        assert len(h) == len(h0) == 25
        dev = np.abs(h - h0) / h0
        print(f"{what}: max rel dev of the history {dev.max():.3e}")
        assert np.all(dev <= np.where(h0 > 1e-4 * h0[0], 1e-8, 5e-2)), dev.max()
        x = np.concatenate([x for x, _ in res])
    else:
        ref, spread = _oracle(oracle, method, N, m, prec, degree if method == "mgsr" else 8, 2)
        h0, xs = single.hist_res, single.x
        assert len({(r.n_out, r.cycles_out, r.n_cycles) for r in res}) == 1
        assert all(np.array_equal(res[0].hist_res, r.hist_res) for r in res)
        mg = np.where(h0 > 1e-10, 1e-5, 1e-3)
        tier = np.where(h0 > 1e-6, 1e-9, mg if method == "mgsr" else np.where(h0 > 1e-12, 1e-3, 5e-2))
        _hist(res[0].hist_res, h0, tier * h0 + 1e-16, spread, what + " vs single context")
        _hist(h0, ref.hist_res, (1e-5 if method == "mgsr" else _hh_oracle(ref.hist_res)) * ref.hist_res + 1e-13, spread,
              what + ": single context vs oracle")
        x = np.concatenate([r.x for r in res])
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    print(f"{what}: max |x - x_single| / max |x_single| {err:.3e}")
    assert err <= 1e-12
