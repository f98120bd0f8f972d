"""Pipelined pass of the w-only MGS-R step with the head of its ring carried across the
all-gather (k_mgs_wres<.., PIPE, CARRY>, GK_TUNE_RES_PIPE_CARRY).

The first chunks of pass p + 1 are loaded inside pass p's all-gather -- wave 0 after it has
published its granule, waves 1..3 ahead of their touches -- and the pass itself then issues
only the rest of its ring.  Loads, their order, the arithmetic and the summation order are
those of the pipelined pass, so every result is bit-identical with the key on or off.  It
runs where the pipelined pass runs: full plans, reached at small size with few workgroups
(GK_TUNE_RES_SHARE = CUs / workgroups):

  N = 512,  4 workgroups:  512 chunks  = 4  x (89 + 39)
  N = 1024, 16 workgroups: 2048 chunks = 16 x (89 + 39)

m = 1 is a single step of two passes (the only head carried into a pass is the closing norm
pass's, whose second load re-reads a chunk of V_i), m = 2 adds the first step with a dot pass
behind a carried head; N = 520 (not full) must report both paths off.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_RES, T_SHARE, T_TMO, T_WONLY, T_PIPE, T_CARRY = 8, 10, 11, 13, 30, 32
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


def _run(N, m, prec, wg, carry, pipe=1, res=1, method="mgsr", cycles=2, memo=True):
    """One solve; (result, res_info of the step's plan, profile).  Computed once per case
    and shared (memo=False: a fresh run, for the determinism check)."""
    import gmres_amd as ga

    key = (N, m, prec, wg, carry, pipe, res, method, cycles)
    if memo and key in _memo:
        return _memo[key]
    with ga.Context(N, m) as c:
        c.tune(T_RES, res)
        c.tune(T_WONLY, 1)
        c.tune(T_SHARE, _workgroups_share(wg))
        c.tune(T_TMO, 5000)
        c.tune(T_PIPE, pipe)
        c.tune(T_CARRY, carry)
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


def _build_carry():
    import gmres_amd as ga

    return ga.res_plan_query(4096 * 4096)["carry"]


def _same(a, b):
    assert a.n_cycles == b.n_cycles
    assert np.array_equal(a.hist_res, b.hist_res), (a.hist_res, b.hist_res)
    assert np.array_equal(a.final_err, b.final_err)
    assert np.array_equal(a.x, b.x)


CASES = [(512, 12, "identity", 4), (512, 1, "identity", 4), (512, 2, "identity", 4), (1024, 8, "cbpr2", 16)]


@pytest.mark.parametrize("N,m,prec,wg", CASES)
def test_carried_step_is_bit_identical(N, m, prec, wg):
    on, pon, prof = _run(N, m, prec, wg, carry=1)
    off, poff, prof_off = _run(N, m, prec, wg, carry=0)
    nopipe, pnp, prof_np = _run(N, m, prec, wg, carry=1, pipe=0)
    for p in (pon, poff, pnp):
        assert p["variant"] == "w-only" and p["G"] == wg and p["r2e"] == RW and p["l2e"] == LW, p
        assert p["nres2"] == N * N // 2, p
    assert pon["pipe"] == 1 and poff["pipe"] == 1 and pnp["pipe"] == 0, (pon, poff, pnp)
    assert pon["carry"] == _build_carry() > 0, pon
    assert poff["carry"] == 0 and pnp["carry"] == 0, (poff, pnp)
    for pr in (prof, prof_off, prof_np):  # the resident launches actually ran
        assert pr["res"][1] > 0, pr
    assert np.all(np.isfinite(on.hist_res)) and np.all(np.isfinite(on.x))
    _same(on, off)
    _same(on, nopipe)


def test_carried_step_is_deterministic():
    a, pa, _ = _run(512, 12, "identity", 4, carry=1)
    b, pb, _ = _run(512, 12, "identity", 4, carry=1, memo=False)
    assert pa["carry"] == pb["carry"] == _build_carry() > 0
    _same(a, b)


def test_default_is_the_builds_choice():
    """-1 (the default) runs what the build selects, with the same results."""
    d, pd, prof = _run(512, 12, "identity", 4, carry=-1, pipe=-1)
    assert pd["carry"] == _build_carry(), pd
    assert prof["res"][1] > 0
    _same(d, _run(512, 12, "identity", 4, carry=1)[0])


def test_householder_chains_unaffected():
    on, pon, prof = _run(512, 12, "identity", 4, carry=1, method="hh")
    off, poff, _ = _run(512, 12, "identity", 4, carry=0, method="hh")
    assert pon["variant"] == "w-only" and pon["pipe"] == 0 and pon["carry"] == 0 and poff["carry"] == 0, (pon, poff)
    assert prof["res"][1] > 0
    _same(on, off)


def test_not_full_plan_carries_nothing():
    """N = 520 on 4 workgroups: 528 chunks and a streamed rest -- not the full case."""
    got, plan, prof = _run(520, 12, "identity", 4, carry=1)
    assert plan["variant"] == "w-only" and plan["pipe"] == 0 and plan["carry"] == 0, plan
    assert prof["res"][1] > 0
    ref, _, _ = _run(520, 12, "identity", 4, carry=1, res=0)
    # the tolerance of test_gpu_wres_pipe.py (test_gpu_resident.py::test_resident_matches_launch_path)
    assert got.n_cycles == ref.n_cycles
    h, r = got.hist_res, ref.hist_res
    tol = np.where(r > 1e-8, 1e-10, 1e-4)
    assert np.all(np.abs(h - r) <= tol * r + 1e-16), (h, r)
    k = min(got.n_out, ref.n_out)
    assert np.allclose(got.final_err[:k], ref.final_err[:k], rtol=1e-6, atol=1e-16)
