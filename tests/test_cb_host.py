"""CPU checks of the compressed-basis feature (gk_set_basis_precision GK_BASIS_F32): the
pure planner of the resident step through gk_cb_plan_query, and the facts of the host
restatement (tests/cb_gmres_host.py) that the GPU tests rest on.  No GPU."""
import os

import numpy as np
import pytest

from tests.cb_gmres_host import CASES, GUARD_CASE, band, case_id, host_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU_LDS = 160 * 1024  # LDS of one CU


# ------------------------------------------------------------------- planner ----

@pytest.mark.parametrize("share", [1, 16, 256])
@pytest.mark.parametrize("nloc", [4, 9, 1089, 16900, 66049, 1024 ** 2, 4096 ** 2])
def test_cb_plan_covers_the_slab(nloc, share):
    import gmres_amd as ga

    p = ga.cb_plan_query(nloc, cus=256, share=share, m=95)
    print(f"nloc {nloc} share {share}: {p}")
    assert p["on"]
    assert p["G"] == 256 // share
    assert p["nres2"] + p["nstream2"] == nloc // 2
    assert p["nres2"] % 256 == 0 and p["nres2"] <= p["G"] * (p["r2e"] + p["l2e"]) * 256
    assert p["lds"] <= CU_LDS - p["lds_static"]
    assert p["lds"] == p["lw"] * 256 * 16  # what the kernel's LDS chunks need
    assert 0 <= p["r2e"] <= p["rw"] and 0 <= p["l2e"] <= p["lw"]


def test_cb_plan_4096_wholly_resident():
    import gmres_amd as ga

    p = ga.cb_plan_query(4096 ** 2, cus=256, share=1, m=95)
    assert p["nstream2"] == 0 and p["nres2"] == 4096 ** 2 // 2
    assert p["r2e"] + p["l2e"] == 128  # 2^23 double2 / 256 workgroups / 256 per chunk


def test_cb_plan_large_m_is_the_launch_path():
    import gmres_amd as ga

    assert not ga.cb_plan_query(4096 ** 2, cus=256, share=1, m=600)["on"]
    assert ga.cb_plan_query(4096 ** 2, cus=256, share=1, m=499)["on"]


def test_cabi_names_of_the_compressed_basis():
    from gmres_amd import _native as nat

    for name in ("gk_set_basis_precision", "gk_get_basis_precision", "gk_cb_plan_query", "gk_set_basis"):
        assert name in nat._SIGS and name in nat.header_symbols()
    hdr = open(os.path.join(ROOT, "include", "gmres_hip.h")).read()
    for line in ("#define GK_BASIS_F64 0", "#define GK_BASIS_F32 1", "#define GK_RES_CB 7",
                 f"#define GK_CB_INFO_LEN {len(nat.CB_INFO_KEYS)}", "#define GK_RES_INFO_LEN 17"):
        assert line in hdr, line
    assert (nat.GK_BASIS_F64, nat.GK_BASIS_F32, nat.GK_RES_CB) == (0, 1, 7)


# --------------------------------------------------- the restatement's own facts --

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f32_basis_keeps_the_cycle_count(oracle, case):
    """The FP32 basis (guarded) takes as many cycles as the FP64 basis, and the
    restatement's own 1-vs-8-thread spread leaves room under the GPU tests' 1e-6 floor:
    100 S_last <= 1e-2 (measured: S_last <= 5.1e-6)."""
    f32 = host_solve(oracle, case, basis="f32")
    f64 = host_solve(oracle, case, basis="f64")
    S = band(oracle, case)
    print(f"{case_id(case)}: cycles f64 {f64.n_cycles} f32 {f32.n_cycles}, last n_out {f64.n_out} / {f32.n_out}, "
          f"S_last {S[-1]:.3e}, guard closed {sum(f32.guarded)} cycles, "
          f"max |x - 1| {np.max(np.abs(f32.x - 1.0)):.3e}")
    assert f32.n_cycles == f64.n_cycles
    assert 100.0 * S[-1] <= 1e-2


def test_unguarded_exit_is_false(oracle):
    """Without the guard the case exits on an estimate far below the true residual
    (measured: estimate / true = 6e-6)."""
    r = host_solve(oracle, GUARD_CASE, guard=False)
    ratio = r.exit_estimate / r.hist_res[-1]
    print(f"unguarded: cycles {r.n_cycles}, estimate {r.exit_estimate:.3e}, true {r.hist_res[-1]:.3e}, ratio {ratio:.3e}")
    assert r.exit_estimate < GUARD_CASE[5]
    assert ratio < 1e-3


def test_guarded_exit_is_true(oracle):
    """With it: two cycles, the exit estimate is the true residual (measured: 7e-4 off),
    and the true residual is below tol."""
    r = host_solve(oracle, GUARD_CASE, guard=True)
    ratio = r.exit_estimate / r.hist_res[-1]
    print(f"guarded: cycles {r.n_cycles}, n_outs {r.n_outs}, estimate {r.exit_estimate:.3e}, "
          f"true {r.hist_res[-1]:.3e}, ratio {ratio:.6f}")
    assert r.n_cycles == 2
    assert r.guarded == [True, False]
    assert abs(ratio - 1.0) <= 1e-2
    assert r.hist_res[-1] < GUARD_CASE[5]
