"""One CGS2 Arnoldi step (gk_set_orthogonalization GK_ORTH_CGS2) on planted, asymmetric columns
against the long-double step of tests/cgs2_data.py.

As in tests/test_gpu_step_known_answer.py a context's cycle is opened, the Krylov columns are
overwritten with the planted near-orthonormal set of tests/general_data.py, step j runs, and
its Hessenberg column and new basis vector are held to the strict bound of step_bounds --
64 eps ||w0|| ||V_i|| per entry of h, 64 eps max |v_ref| per element of the column -- against
cgs2_step(V, w0) in long double, w0 from the oracle's operators (bit-exact with the device's).
tests/test_cgs2_data.py pins on the CPU that a float64 CGS2 step with another summation tree
stays below 1/8 of that bound and that a skipped sweep, a dropped tail element of the dots or
of one AXPY column, a dropped 512-element chunk and a zeroed dot all exceed it.  CGS2 differs
from the strict MGS-R step far outside the bound on these columns (second order in the Gram
off-diagonals), so a device that ran the MGS-R chain instead fails here.

Covered: the launch chain call by call and as a replayed hipGraph; a full batch of KB columns,
a ragged one and odd n; 1 and 3 workgroups (several grid-stride trips, partial slabs of length
1 and 3); m above the resident limit of 512; both batch sizes of the dots kernel; every
preconditioner route on either side; three uneven ranks over the local group's collectives and
over the device exchange.
"""
import contextlib
import os
import threading

import numpy as np
import pytest

from tests import cgs2_data as cd
from tests.general_data import PARAMS, PREC_STEP_CASES, check_step, op_w0, plant, read_col

pytestmark = pytest.mark.gpu


def _nat():
    from gmres_amd import _native as nat

    return nat


def _ref(oracle, N, m, j, op=None):
    if op is None:
        return cd.step_ref(N, m, j, w0_of=lambda v: oracle.stvec(v, N), key="A")
    return cd.step_ref(N, m, j, w0_of=lambda v: op_w0(oracle, v, N, *op), key=op)


@contextlib.contextmanager
def _batch_env(kb):
    """GK_CGS_KB = kb in the environment (None: untouched) while a context is created."""
    old = os.environ.get("GK_CGS_KB")
    if kb is not None:
        os.environ["GK_CGS_KB"] = str(kb)
    try:
        yield
    finally:
        if kb is not None:
            if old is None:
                del os.environ["GK_CGS_KB"]
            else:
                os.environ["GK_CGS_KB"] = old


def _open(N, m, tunes, side="left", prec=("identity", 1), kb=None, params=PARAMS):
    """A CGS2 context with its tuning applied and an MGS-R cycle open; every column planted.
    kb: the dots kernel's batch, which gk_create reads from GK_CGS_KB."""
    import gmres_amd as ga

    with _batch_env(kb):
        c = ga.Context(N, m)
    try:
        for k, v in tunes:
            c.tune(k, v)
        c.set_precond(prec[0], params, prec[1], side=side)
        c.set_orth("cgs2")
        c.set_rhs_ones()
        c.mgs_cycle_start()
        V = cd.planted(N, m)
        for k in range(m):
            plant(c, k, V[k])
    except Exception:
        c.close()
        raise
    return c


def _step(c, N, m, j):
    h = c.mgs_step(j)
    v = read_col(c, j)
    if j < m:
        plant(c, j, cd.planted(N, m)[j])
    return h, v


def _check(oracle, c, N, m, js, what, twice=False, op=None):
    """Steps js (each twice where the second run is to be a graph replay), each held to the
    strict bound; returns the number of steps run."""
    worst, steps = (0.0, 0.0), 0
    for j in js:
        V, w0, ref = _ref(oracle, N, m, j, op)
        for rep in range(2 if twice else 1):
            h, v = _step(c, N, m, j)
            steps += 1
            r = check_step(h, v, V, w0, ref, f"{what} N={N} m={m} j={j}" + (" (replay)" if rep else ""))
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"{what} N={N} m={m}: worst h dev/bound {worst[0]:.3e}, column dev/bound {worst[1]:.3e}")
    return steps


def _base_cases():
    KB = _nat().GK_CGS_KB
    return [(2, 3, (1, 2, 3)), (3, 5, (1, 2, 5)), (45, 12, (1, 2, 12)), (130, 6, (1, 2, 6)),
            (33, 2 * KB + 1, (KB, KB + 1, 2 * KB + 1))]  # a full batch, a ragged one, odd n


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("case", range(5))
def test_cgs2_step(oracle, case, graph):
    """The chain call by call (4 projection-class launches per step: dots, AXPY, dots, AXPY)
    and as a hipGraph: every step twice, re-planted in between -- the second run is a replay."""
    nat = _nat()
    N, m, js = _base_cases()[case]
    c = _open(N, m, [(nat.GK_TUNE_GRAPH, graph)])
    with c:
        assert c.orth == "cgs2" and c.res_info()["variant"] is None
        c.profile(True)
        c.profile_reset()
        steps = _check(oracle, c, N, m, js, f"cgs2 graph={graph}", twice=bool(graph))
        prof = c.profile_read()
    assert prof["res"][1] == 0, prof
    if graph:
        assert prof["graph"][1] == steps and prof["proj"][1] == 0, prof
    else:
        assert prof["graph"][1] == 0 and prof["proj"][1] == 4 * steps, prof
        assert prof["other"][1] >= 2 * steps, prof  # the two fixed-order reduces


@pytest.mark.parametrize("blocks", [1, 3])
def test_cgs2_step_workgroup_counts(oracle, blocks):
    """GK_TUNE_PROJ_BLOCKS 1 and 3 at N = 130: 33 and 11 grid-stride trips per thread, partial
    slabs of length 1 and 3."""
    nat = _nat()
    N, m = 130, 6
    c = _open(N, m, [(nat.GK_TUNE_PROJ_BLOCKS, blocks), (nat.GK_TUNE_GRAPH, 0)])
    with c:
        _check(oracle, c, N, m, [1, 2, m], f"cgs2 blocks={blocks}")


@pytest.mark.parametrize("kb", [8, 16])
def test_cgs2_step_large_m(oracle, kb):
    """m = 520, above the resident step's limit of 512: steps 513 and 520 (s staged in LDS and
    the slab sized from j and m, not from 512), with batches of 8 and of 16 columns."""
    N, m = 32, 520
    c = _open(N, m, [], kb=kb)
    with c:
        _check(oracle, c, N, m, [513, 520], f"cgs2 large m KB={kb}")


def test_cgs2_step_batches_of_16(oracle):
    """The KB = 16 instantiation on odd n: a full batch, a ragged one, two batches and a column."""
    nat = _nat()
    N, m = 33, 33
    c = _open(N, m, [(nat.GK_TUNE_GRAPH, 0)], kb=16)
    with c:
        _check(oracle, c, N, m, [16, 17, 33], "cgs2 KB=16")


@pytest.mark.parametrize("case", PREC_STEP_CASES, ids=[c[0] for c in PREC_STEP_CASES])
def test_cgs2_preconditioned_step(oracle, case):
    """Every preconditioner route on either side in front of the CGS2 chain (the operator stage
    without its fused first dot, except Chebyshev on the left, whose slab stays unconsumed)."""
    nat = _nat()
    _, side, kind, degree, named, N, m, params = case
    tunes = [(getattr(nat, k), v) for k, v in named]
    c = _open(N, m, tunes, side=side, prec=(kind, degree), params=params)
    with c:
        assert c.res_info()["variant"] is None
        _check(oracle, c, N, m, [1, 2, m], f"cgs2 {case[0]}", op=(side, kind, degree, params))


def test_batch_knob_rejects_other_sizes():
    import gmres_amd as ga

    with _batch_env(12):
        with pytest.raises(Exception, match="GK_CGS_KB"):
            ga.Context(16, 4)


@pytest.mark.parametrize("mode", ["local-group", "device-exchange"])
def test_cgs2_three_rank_step(oracle, mode):
    """N = 130 over three uneven LocalGroup ranks on one GPU, one host thread per rank: the
    all-reduces of s and of the norm slab through the local group's collectives, and through
    the device exchange (k_xchg vector exchanges inside the replayed graph).  Every rank
    reports the same h; the concatenated column is held to the bound."""
    import gmres_amd as ga

    nat = _nat()
    N, m, R = 130, 6, 3
    js = [1, 2, m]
    parts = ga.slab_partition(N, R)
    assert len({nl for _, nl in parts}) > 1  # uneven
    V = cd.planted(N, m)
    g = ga.LocalGroup(R)
    ctxs = [ga.Context(N, m, device=0, line0=l0, nlines=nl) for l0, nl in parts]
    out, err = [None] * R, []
    bar = threading.Barrier(R)
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_local(g, r, max(nl for _, nl in parts))
        if mode == "device-exchange":
            for c in ctxs:
                c.xchg_local()
                c.tune(nat.GK_TUNE_RES, 0)
                c.tune(nat.GK_TUNE_GRAPH, 1)
                c.tune(nat.GK_TUNE_XCHG_TIMEOUT_MS, 5000)

        def work(r):
            try:
                c = ctxs[r]
                lo, hi = parts[r][0] * N, (parts[r][0] + parts[r][1]) * N
                c.set_precond("identity")
                c.set_orth("cgs2")
                c.set_rhs_ones()
                c.mgs_cycle_start()
                for k in range(m):
                    plant(c, k, V[k, lo:hi])
                assert c.res_info()["variant"] is None
                c.profile(True)
                c.profile_reset()
                res = []
                for j in js:
                    bar.wait(timeout=60)  # every rank's columns are in place
                    h = c.mgs_step(j)
                    v = read_col(c, j)
                    bar.wait(timeout=60)  # every rank has read before anyone re-plants
                    if j < m:
                        plant(c, j, V[j, lo:hi])
                    res.append((h, v))
                out[r] = (res, c.profile_read())
            except Exception as e:  # pragma: no cover - reported below
                bar.abort()
                err.append(e)

        th = [threading.Thread(target=work, args=(r,)) for r in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
        assert not err, err
        assert all(o is not None for o in out)
    finally:
        for c in ctxs:
            c.close()
        g.close()
    for r in range(R):
        prof = out[r][1]
        assert prof["res"][1] == 0, prof
        if mode == "device-exchange":
            assert prof["graph"][1] == len(js), prof
        else:
            assert prof["proj"][1] == 4 * len(js) and prof["comm"][1] >= 3 * len(js), prof
    for i, j in enumerate(js):
        Vj, w0, ref = _ref(oracle, N, m, j)
        hs = [out[r][0][i][0] for r in range(R)]
        assert all(np.array_equal(hs[0], h) for h in hs[1:]), hs
        v = np.concatenate([out[r][0][i][1] for r in range(R)])
        check_step(hs[0], v, Vj, w0, ref, f"cgs2 {mode} j={j}")
