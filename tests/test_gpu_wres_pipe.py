"""Software-pipelined pass of the w-only MGS-R step (k_mgs_wres<.., PIPE>, GK_TUNE_RES_PIPE).

The pipelined pass keeps the column loads of the next 7 chunks in flight while it waits,
with a counted wait, for the chunk it consumes, so it runs only where every workgroup holds
its full 89 + 39 chunks of 256 double2 and nothing is streamed.  The smallest such slabs are
reached with few workgroups (GK_TUNE_RES_SHARE = CUs / workgroups):

  N = 512,  4 workgroups:  512 chunks  = 4  x (89 + 39)
  N = 1024, 16 workgroups: 2048 chunks = 16 x (89 + 39)

The per-thread arithmetic and the summation order are those of the batch-by-batch pass,
so every result is bit-identical with the key on or off; N = 520 (not full) must report
the pipelined path off and run the present code.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_RES, T_SHARE, T_TMO, T_WONLY, T_PIPE = 8, 10, 11, 13, 30
RW, LW = 89, 39

_cus = []
_memo = {}


def _workgroups_share(wg):
    """GK_TUNE_RES_SHARE that leaves `wg` workgroups: CUs / wg (a forced w-only plan runs
    CUs / share workgroups; at 2048^2 with share 1 that is one per CU)."""
    import gmres_amd as ga

    if not _cus:
        with ga.Context(2048, 2) as c:
            c.tune(T_RES, 1)
            c.tune(T_WONLY, 1)
            plan = c.res_info()
        assert plan["variant"] == "w-only", plan
        _cus.append(plan["G"])
    assert _cus[0] % wg == 0, _cus
    return _cus[0] // wg


def _run(N, m, prec, wg, pipe, res=1, method="mgsr", cycles=2, memo=True):
    """One solve; (result, res_info of the step's plan, profile).  Computed once per case
    and shared (memo=False: a fresh run, for the determinism check)."""
    import gmres_amd as ga

    key = (N, m, prec, wg, pipe, res, method, cycles)
    if memo and key in _memo:
        return _memo[key]
    with ga.Context(N, m) as c:
        c.tune(T_RES, res)
        c.tune(T_WONLY, 1)
        c.tune(T_SHARE, _workgroups_share(wg))
        c.tune(T_TMO, 5000)
        c.tune(T_PIPE, pipe)
        c.set_precond(prec, (8.2, 0.2), 4)
        c.set_rhs_ones()
        c.profile(True)
        c.profile_reset()
        if method == "hh":
            r = ga.gmres_hh(c, 1e-15, precondition=(prec != "identity"), max_cycles=cycles, want_hist=True)
        else:
            r = ga.gmres_mgsr(c, 1e-15, max_cycles=cycles, want_hist=True)
        out = (r, c.res_info(hh=method == "hh"), c.profile_read())
    if memo:
        _memo[key] = out
    return out


def _same(a, b):
    assert a.n_cycles == b.n_cycles
    assert np.array_equal(a.hist_res, b.hist_res), (a.hist_res, b.hist_res)
    assert np.array_equal(a.final_err, b.final_err)
    assert np.array_equal(a.x, b.x)


@pytest.mark.parametrize("N,m,prec,wg", [(512, 12, "identity", 4), (1024, 8, "cbpr2", 16)])
def test_pipelined_step_is_bit_identical(N, m, prec, wg):
    on, pon, prof = _run(N, m, prec, wg, pipe=1)
    off, poff, prof_off = _run(N, m, prec, wg, pipe=0)
    for p in (pon, poff):
        assert p["variant"] == "w-only" and p["G"] == wg and p["r2e"] == RW and p["l2e"] == LW, p
        assert p["nres2"] == N * N // 2, p
    assert pon["pipe"] == 1 and poff["pipe"] == 0, (pon, poff)
    # the resident launches ran every step (k_proj only in the off-cycle diagnostics)
    for pr in (prof, prof_off):
        assert pr["res"][1] > 0 and pr["proj"][1] < pr["res"][1] // 4, pr
    assert np.all(np.isfinite(on.hist_res)) and on.hist_res[-1] < on.hist_res[0]
    _same(on, off)


def test_pipelined_step_is_deterministic():
    a, pa, _ = _run(512, 12, "identity", 4, pipe=1)
    b, pb, _ = _run(512, 12, "identity", 4, pipe=1, memo=False)
    assert pa["pipe"] == 1 and pb["pipe"] == 1
    _same(a, b)


def test_default_is_the_builds_choice():
    """-1 (the default) runs what the build selects, with the same results."""
    import gmres_amd as ga

    d, pd, _ = _run(512, 12, "identity", 4, pipe=-1)
    assert pd["pipe"] == ga.res_plan_query(4096 * 4096)["pipe"]
    _same(d, _run(512, 12, "identity", 4, pipe=1)[0])


def test_householder_chains_unaffected():
    on, pon, prof = _run(512, 12, "identity", 4, pipe=1, method="hh")
    off, poff, _ = _run(512, 12, "identity", 4, pipe=0, method="hh")
    assert pon["variant"] == "w-only" and pon["pipe"] == 0 and poff["pipe"] == 0, (pon, poff)
    assert prof["res"][1] > 0
    _same(on, off)


def _close_to_launch_path(got, ref):
    # the tolerance of test_gpu_resident.py::test_resident_matches_launch_path
    assert got.n_cycles == ref.n_cycles
    h, r = got.hist_res, ref.hist_res
    tol = np.where(r > 1e-8, 1e-10, 1e-4)
    assert np.all(np.abs(h - r) <= tol * r + 1e-16), (h, r)
    k = min(got.n_out, ref.n_out)
    assert np.allclose(got.final_err[:k], ref.final_err[:k], rtol=1e-6, atol=1e-16)


def test_not_full_plan_keeps_the_present_pass():
    """N = 520 on 4 workgroups: 528 chunks and a streamed rest -- not the full case."""
    got, plan, prof = _run(520, 12, "identity", 4, pipe=1)
    assert plan["variant"] == "w-only" and plan["pipe"] == 0, plan
    assert prof["res"][1] > 0
    ref, _, _ = _run(520, 12, "identity", 4, pipe=1, res=0)
    _close_to_launch_path(got, ref)


def test_pipelined_step_matches_launch_path():
    got, plan, _ = _run(512, 12, "identity", 4, pipe=1)
    assert plan["pipe"] == 1
    ref, _, _ = _run(512, 12, "identity", 4, pipe=1, res=0)
    _close_to_launch_path(got, ref)
