"""The multigrid preconditioner (GK_PREC_MG) without a GPU: the level and coarse-degree
rules of the restatement (tests/mg_data.py) and of the library's host planner, the
restated cycle's symmetry, positivity and PCG iteration counts, and the C-ABI's surface."""
import ctypes
import os

import numpy as np
import pytest

from tests import mg_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVELS = {16: [16, 8], 20: [20, 10], 48: [48, 24, 12], 100: [100, 50, 25], 130: [130, 65], 514: [514, 257],
          4096: [4096, 2048, 1024, 512, 256, 128, 64, 32, 16, 8]}
COARSE_DEGREE = {**{n: n for n in range(8, 17)}, 24: 23, 25: 24, 257: 64, 513: 64}


@pytest.fixture(scope="module")
def built():
    from gmres_amd import build

    build.build_all()
    from gmres_amd import _native

    return _native


def test_restatement_levels_and_coarse_degree():
    for N, sides in LEVELS.items():
        assert mg_data.levels(N) == sides
    for NL, nu in COARSE_DEGREE.items():
        lo, hi, nuc = mg_data.coarse(NL)
        assert nuc == nu, (NL, nuc)
        assert 0.0 < lo < hi < 8.0
    assert mg_data.levels(127) == [127] and mg_data.levels(14) == [14]  # no coarse level


def test_plan_query_levels_and_coarse_degree(built):
    """gk_mg_plan_query is pure host: the same rules, no device touched."""
    import gmres_amd as ga

    for N, sides in LEVELS.items():
        plan = ga.mg_plan(N)
        assert plan == {"levels": len(sides), "sides": sides, "coarse_degree": mg_data.coarse(sides[-1])[2]}
    for NL, nu in COARSE_DEGREE.items():  # where 2 NL halves once, to a last level of side NL
        plan = ga.mg_plan(2 * NL)
        if plan["sides"][-1] == NL:
            assert plan["coarse_degree"] == nu, NL
    L = built.hip()
    info = (ctypes.c_int * built.GK_MG_INFO_LEN)()
    for bad in (127, 14, 2, 0, -4):
        assert L.gk_mg_plan_query(bad, info) == built.GK_ERR_ARG, bad
    assert L.gk_mg_plan_query(64, None) == built.GK_ERR_ARG


def test_null_context_calls_are_argument_errors(built):
    L = built.hip()
    info = (ctypes.c_int * built.GK_MG_INFO_LEN)()
    v = np.zeros(4)
    p = v.ctypes.data_as(built._dp)
    assert L.gk_mg_info(None, info) == built.GK_ERR_ARG
    assert L.gk_mg_transfer(None, 0, 0, p, p, p) == built.GK_ERR_ARG
    pr = np.array([8.0, 1.0])
    assert L.gk_set_precond(None, built.GK_PREC_MG, pr.ctypes.data_as(built._dp), 2, 2) == built.GK_ERR_ARG


def test_surface(built):
    hdr = open(built.HEADER).read()
    assert "#define GK_PREC_MG 3" in hdr and "#define GK_TUNE_MG_FUSED 33" in hdr
    assert f"#define GK_MG_INFO_LEN {built.GK_MG_INFO_LEN}" in hdr
    assert built.GK_PREC_MG == 3 and built.GK_TUNE_MG_FUSED == 33
    assert built._SIGS["gk_mg_plan_query"] == (built.c_int, [built.c_int, built._ip])
    assert built._SIGS["gk_mg_info"] == (built.c_int, [built.c_vp, built._ip])
    assert built._SIGS["gk_mg_transfer"] == (built.c_int, [built.c_vp, built.c_int, built.c_int, built._dp, built._dp,
                                                             built._dp])
    for name in ("gk_mg_plan_query", "gk_mg_info", "gk_mg_transfer"):
        assert name in built.header_symbols() and hasattr(built.hip(), name)
    import gmres_amd.solver as S
    from gmres_amd import build as b

    assert S.PREC["mg"] == S.PREC["multigrid"] == 3
    assert [u[2] for u in b.HIP_UNITS_MG] == ["gk_mg.o"]
    out = __import__("subprocess").run(["nm", "-D", built.FHOST_SO], capture_output=True, text=True).stdout
    assert "hip_mg" in out
    exe = os.path.join(ROOT, "gmres_amd", "lib", "test_mfp_hip")
    assert "|mg]" in __import__("subprocess").run([exe], capture_output=True, text=True, timeout=60).stdout


def test_set_precond_defaults_by_kind(monkeypatch):
    """Context.set_precond resolves its defaults per kind: "mg" takes (8, 1) and degree 2,
    every other call keeps (8.2, 0.2) and 8."""
    import gmres_amd.solver as S

    seen = []

    class FakeLib:
        def gk_set_precond(self, h, k, p, n, degree):
            seen.append((k, [p[i] for i in range(n)], degree))
            return 0

    monkeypatch.setattr(S.nat, "hip", lambda: FakeLib())
    c = object.__new__(S.Context)
    c._h, c.side = None, "left"
    c.set_precond("mg")
    c.set_precond("cheb")
    c.set_precond("cbpr2", (8.1, 0.3))
    c.set_precond("mg", (8.2, 2.0), 3)
    c.set_precond("cheb", degree=4)
    assert seen == [(3, [8.0, 1.0], 2), (2, [8.2, 0.2], 8), (1, [8.1, 0.3], 8), (3, [8.2, 2.0], 3), (2, [8.2, 0.2], 4)]


@pytest.mark.parametrize("N", [16, 48, 100])
def test_restated_cycle_is_symmetric_positive(oracle, N):
    """<M^-1 u, v> = <u, M^-1 v> to a relative 1e-11 (the coarsest level's sweep count
    amplifies rounding), and <u, M^-1 u> > 0, on random vectors."""
    rng = np.random.default_rng(N)
    for _ in range(3):
        u, v = rng.standard_normal(N * N), rng.standard_normal(N * N)
        mu, mv = mg_data.mg(oracle, u, N), mg_data.mg(oracle, v, N)
        asym = abs(float(mu @ v) - float(u @ mv)) / abs(float(mu @ v))
        print(f"N={N} asymmetry {asym:.3e}")
        assert asym <= 1e-11
        assert float(u @ mu) > 0.0 and float(v @ mv) > 0.0


@pytest.mark.parametrize("N,iters", [(16, 7), (48, 8), (100, 8), (128, 9)])
def test_restated_pcg_iteration_counts(oracle, N, iters):
    """b = A 1, x0 = 0, to ||r|| / ||b|| < 1e-8 with the defaults (degree 2 on (8, 1))."""
    it, rel = mg_data.pcg(oracle, N)
    print(f"N={N} iterations {it} rel {rel:.3e}")
    assert rel < 1e-8
    assert abs(it - iters) <= 1
