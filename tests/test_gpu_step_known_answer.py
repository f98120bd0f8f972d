"""One Arnoldi step on planted, asymmetric columns against a long-double step
(tests/general_data.py).

Every other step-level test feeds the device b = A*1, whose Krylov vectors equal their own
index reversal, transposed grid and line-reversed grid, and judges the step by residual
histories, which GMRES's self-correction flattens.  Here a context's cycle is opened, the
Krylov columns 0..j-1 are overwritten with a planted near-orthonormal set that has none of
the symmetries (Gram off-diagonals ~1e-3 / N: both MGS passes and the norm carry signal), step j
runs, and its Hessenberg column and new basis vector are held to

    |h_i - h_ref_i|        <= 64 eps ||w0|| ||V_i||   (||V_i|| = 1 for h_{j+1})
    max |v_new - v_ref|    <= 64 eps max |v_ref|

with (h_ref, v_ref) = mgs_step_ld(V, w0), w0 = oracle.stvec(V_{j-1}) (bit-exact with the
device stencil, test_poisson5_bitexact).  eps ||w|| ||v|| is the first-order rounding error
of a dot under any summation tree; tests/test_general_data.py pins on the CPU that a
reordered float64 step stays below 1/8 of the bound and that a dropped tail element, a
dropped 512-element chunk of one AXPY and a skipped second pass exceed it.

A step reads V(:,j) and every column from HBM, so planting after gk_mgs_cycle_start is
valid; the blocked step (GK_TUNE_RES_BLOCK) also reads Gram rows that the earlier blocked
steps of the cycle wrote, so there the steps 1..j run in order, each output column
re-planted, and every one of them is checked.

The blocked step does not meet the strict bound on planted columns: its second sweep visits
the blocks in reverse order, which changes the result at second order in the Gram
off-diagonals (nothing on an orthonormal basis).  Its bound against mgs_step_ld is therefore
8 x the deviation of its float64 emulation (general_data.blocked_step, numpy on the same
planted data) from mgs_step_ld, never below the strict bound; on the CPU that deviation is
4e3 .. 5e5 (h) and 1.4e4 .. 1.3e6 (column) times the strict bound at N = 256 .. 45
(tests/test_general_data.py::test_blocked_step_emulation).  Because that is wide, the blocked
step is also held to the STRICT bound against the long-double evaluation of its own order.

test_preconditioned_step runs the step behind cbpr2 and Chebyshev(k) on either side, where the
first dot <w, V(:,1)> comes from the operator launch's epilogue instead of the stencil's; the
FP32-basis step has the same cases in test_gpu_cb_step_known_answer.py.

The same planted contexts check gk_update_x, gk_mgs_verr, gk_vec_dot and the gk_vec_lincomb
forms against long-double / exact float64 evaluations.
"""
import ctypes
import threading

import numpy as np
import pytest

from tests import test_gpu_blocked as tb
from tests import test_gpu_resident as tr
from tests.general_data import (PREC_STEP_CASES, EPS, MARGIN, PARAMS, blocked_step, check_step, mgs_step_ld, op_w0, plant,
                                planted_basis, read_col, step_bounds)

pytestmark = pytest.mark.gpu

T_RES, T_R2, T_SHARE, T_TMO, T_WONLY, T_GRAPH, T_PC, T_FOLD, T_PIPE, T_CARRY = 8, 9, 10, 11, 13, 19, 21, 22, 30, 32
T_VERR_ORDER = 14

_basis: dict = {}
_refs: dict = {}


def _V(N, m):
    """The planted columns of an (N, m) context, rows 0..m-1; once per shape."""
    if (N, m) not in _basis:
        _basis[(N, m)] = planted_basis(N, m, seed=5000 + 7 * N + m)
    return _basis[(N, m)]


def _ref(oracle, N, m, j, op=None):
    """(V[:j], w0, (h_ref, v_ref)) of step j on the planted columns; once per case.
    op = (side, kind, degree, params): the preconditioned operator instead of A."""
    key = (N, m, j) if op is None else (N, m, j, op)
    if key not in _refs:
        V = _V(N, m)[:j]
        w0 = oracle.stvec(V[j - 1], N) if op is None else op_w0(oracle, V[j - 1], N, *op)
        _refs[key] = (V, w0, mgs_step_ld(V, w0))
    return _refs[key]


def _blk_ref(N, m, j, S, V, w0):
    """The blocked step's order of operations on the planted columns: (long double, float64)."""
    key = (N, m, j, S)
    if key not in _refs:
        _refs[key] = (blocked_step(V, w0, S), blocked_step(V, w0, S, dtype=np.float64))
    return _refs[key]


def _open(N, m, tunes, side="left", prec=("identity", 1), params=PARAMS, **kw):
    """A context with its tuning applied and an MGS-R cycle open on the identity
    preconditioner (or prec = (kind, degree) on `params`); every column 0..m-1 planted."""
    import gmres_amd as ga

    c = ga.Context(N, m, **kw)
    try:
        for k, v in tunes:
            c.tune(k, v)
        c.set_precond(prec[0], params, prec[1], side=side)
        c.set_rhs_ones()
        c.mgs_cycle_start()
        V = _V(N, m)
        for k in range(m):
            plant(c, k, V[k])
    except Exception:
        c.close()
        raise
    return c


def _step(c, N, m, j):
    """Step j on the planted columns; the output column is then planted again so that a
    later step of the same context sees the planted set."""
    h = c.mgs_step(j)
    v = read_col(c, j)
    if j < m:
        plant(c, j, _V(N, m)[j])
    return h, v


def _check(oracle, c, N, m, js, what, twice=False, op=None):
    worst = (0.0, 0.0)
    plan = c.res_info()
    for j in js:
        V, w0, ref = _ref(oracle, N, m, j, op)
        for rep in range(2 if twice else 1):
            h, v = _step(c, N, m, j)
            r = check_step(h, v, V, w0, ref, f"{what} N={N} m={m} j={j}" + (" (replay)" if rep else ""), plan=plan)
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"{what} N={N} m={m}: worst h dev/bound {worst[0]:.3e}, column dev/bound {worst[1]:.3e}")
    return worst


# ---------------------------------------------------------------- launch path ---

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("N,m", [(2, 3), (3, 5), (45, 12), (130, 6)])
def test_launch_path_step(oracle, N, m, graph):
    """One launch per projection (GK_TUNE_RES 0), call by call and as a hipGraph; on the
    graph route every step runs twice, re-planted in between: the second is a replay.
    j = 1 (no earlier column), 2 and m (every column)."""
    c = _open(N, m, [(T_RES, 0), (T_GRAPH, graph)])
    with c:
        assert c.res_info()["variant"] is None
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, [1, 2, m], f"launch graph={graph}", twice=bool(graph))
        prof = c.profile_read()
    assert prof["res"][1] == 0, prof
    if graph:
        assert prof["graph"][1] > 0, prof
    else:
        assert prof["graph"][1] == 0 and prof["proj"][1] > 0, prof


# ----------------------------------------------------------- resident variants ---

RES_CASES = ([(c[0], c[1], c[3], c[4], -1, -1, "prefetch") for c in tr.CASES if c[0] <= 512]
             + [(c[0], c[1], c[3], c[4], 1, 0, "w-only") for c in tr.WCASES]
             + [(c[0], c[1], c[3], c[4], -1, 1, "w+column") for c in tr.PCASES]
             # the two-array variant, which none of those tuples selects below N = 700: more than 8
             # chunks of 448 per workgroup, without (pairs) and with (pairs+lds, the other large-slab
             # variants switched off) chunks beyond 12 x 512 per workgroup; odd N, streamed tails
             + [(181, 16, 0, 64, -1, -1, "pairs"), (300, 20, 0, 32, -1, -1, "pairs"),
                (181, 16, 0, 128, 0, 0, "pairs+lds"), (300, 20, 0, 64, 0, 0, "pairs+lds"),
                (512, 24, 0, 32, 0, 0, "pairs+lds")])


def _res_tunes(r2, share, wonly, pc):
    return [(T_PC, pc), (T_RES, 1), (T_WONLY, wonly), (T_R2, r2), (T_SHARE, share), (T_TMO, 5000)]


@pytest.mark.parametrize("N,m,r2,share,wonly,pc,variant", RES_CASES)
def test_resident_step(oracle, N, m, r2, share, wonly, pc, variant):
    """The forcing tuples of test_gpu_resident.py up to N = 512 (prefetch R2 2 / 4 / 8, w-only,
    w+column) and five more for pairs and pairs+LDS; odd N, streamed tails; j = 1, 5 and m."""
    c = _open(N, m, _res_tunes(r2, share, wonly, pc))
    with c:
        plan = c.res_info()
        print(f"resident N={N} m={m} r2={r2} share={share} wonly={wonly} pc={pc}: {plan}")
        assert plan["variant"] == variant, plan
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, [1, 5, m], f"resident {plan['variant']}")
        prof = c.profile_read()
    assert prof["res"][1] >= 3 and prof["proj"][1] == 0, prof


@pytest.mark.parametrize("pipe,carry", [(1, 1), (1, 0), (0, 0)])
def test_pipelined_and_carried_pass(oracle, pipe, carry):
    """The w-only step's software-pipelined pass, with and without the head of its ring
    carried across the all-gather, and the batch-by-batch pass on the same full plan
    (N = 512 on 4 workgroups: 4 x (89 + 39) chunks, nothing streamed)."""
    import gmres_amd as ga
    from tests.test_gpu_wres_carry import _workgroups_share

    N, m, wg = 512, 12, 4
    tunes = [(T_RES, 1), (T_WONLY, 1), (T_SHARE, _workgroups_share(wg)), (T_TMO, 5000), (T_PIPE, pipe),
             (T_CARRY, carry)]
    c = _open(N, m, tunes)
    with c:
        plan = c.res_info()
        print(f"pipe={pipe} carry={carry}: {plan}")
        assert plan["variant"] == "w-only" and plan["G"] == wg and plan["r2e"] == 89 and plan["l2e"] == 39, plan
        assert plan["nres2"] == N * N // 2 and plan["pipe"] == pipe, plan
        if carry:
            assert plan["carry"] == ga.res_plan_query(4096 * 4096)["carry"] > 0, plan
        else:
            assert plan["carry"] == 0, plan
        _check(oracle, c, N, m, [1, 5, m], f"w-only pipe={pipe} carry={carry}")


# ---------------------------------------------------------------- blocked step ---

# share -> the k_mgs_blk build a 512^2 slab selects with 256 / share workgroups: the chunks of
# 512 double2 per workgroup that test_gpu_blocked.SHARES reaches at 1024^2 (4 / 8 / 16 / 32
# register chunks, then the w-only build)
BLK_SHARES = [4 * s for s, _, _ in tb.SHARES]
BLK_CASES = ([(512, 6, S, sh, 0) for S in (2, 4) for sh in BLK_SHARES]
             + [(127, 6, S, 1, 0) for S in (2, 4)]   # odd n (tail element), partial chunks
             + [(512, 6, 1, BLK_SHARES[1], 1)])       # the strict step on the prefetching build


@pytest.mark.parametrize("N,m,S,share,pf", BLK_CASES)
def test_blocked_step(oracle, N, m, S, share, pf):
    """k_mgs_blk, S = 2 / 4 (and S = 1 with GK_TUNE_RES_PF), every build; steps 1..6 in order
    (partial and full blocks: j - 1 = 0, 1, 4, 5 columns after V_1 among them).  S > 1: the
    emulation bound against the strict step and the strict bound against the blocked order
    (module docstring); S = 1: the strict bound."""
    from gmres_amd import _native as nat

    tunes = [(nat.GK_TUNE_RES_PF, 1)] if pf else [(nat.GK_TUNE_RES_BLOCK, S)]
    if share > 1:
        tunes += [(T_RES, 1), (T_SHARE, share)]
    tunes += [(T_TMO, 10000)]
    c = _open(N, m, tunes)
    with c:
        plan = c.res_info()
        print(f"blocked N={N} S={S} share={share} pf={pf}: {plan}")
        assert plan["variant"] == "blocked" and plan["blk"] == S, plan
        if N == 512:
            assert plan["G"] == 256 // share, plan
        c.profile(True)
        c.profile_reset()
        what = f"blocked S={S} share={share} pf={pf}"
        if S == 1:  # the strict order on the blocked kernel
            _check(oracle, c, N, m, list(range(1, m + 1)), what)
        for j in range(1, m + 1 if S > 1 else 1):
            V, w0, strict = _ref(oracle, N, m, j)
            own, emu = _blk_ref(N, m, j, S, V, w0)
            hb, vb = step_bounds(V, w0, strict[1])
            wide = (np.maximum(hb, 8.0 * np.abs(emu[0] - strict[0])), max(vb, 8.0 * np.max(np.abs(emu[1] - strict[1]))))
            h, v = _step(c, N, m, j)
            check_step(h, v, V, w0, strict, f"{what} N={N} j={j} vs strict step, emulation bound", bounds=wide, plan=plan)
            check_step(h, v, V, w0, own, f"{what} N={N} j={j} vs blocked order, strict bound", plan=plan)
        prof = c.profile_read()
    assert prof["res"][1] >= m and prof["proj"][1] == 0, prof


# -------------------------------------------------------- right side, identity ---

def test_right_identity_step_is_the_left_step(oracle):
    N, m = 130, 6
    out = {}
    for side in ("left", "right"):
        c = _open(N, m, [], side=side)
        with c:
            out[side] = [_step(c, N, m, j) for j in (1, 5)]
    for (hl, vl), (hr, vr), j in zip(out["left"], out["right"], (1, 5)):
        assert np.array_equal(hl, hr) and np.array_equal(vl, vr)
        V, w0, ref = _ref(oracle, N, m, j)
        check_step(hr, vr, V, w0, ref, f"right identity N={N} j={j}")


# ----------------------------- the first dot from the operator launch's epilogue ---

@pytest.mark.parametrize("route", ["launch", "resident"])
@pytest.mark.parametrize("case", PREC_STEP_CASES, ids=[c[0] for c in PREC_STEP_CASES])
def test_preconditioned_step(oracle, case, route):
    """Every case above runs on the identity, whose first dot <w, V(:,1)> is the stencil's.
    With a preconditioner it comes from the operator launch's epilogue: cbpr2, the Chebyshev
    pass's ACC_DOT over overlapping windows (one fused pass, two passes, per-sweep kernels;
    the stencil as stage 0 of the pass and as a launch of its own), k_right_cbpr2 and its
    two-launch form, Chebyshev(3) on the right.  w0 is the oracle's M^-1 A v (right: A M^-1 v),
    bit-exact with the device operators; the bounds are the identity cases'.  j = 1, 2, m on
    the launch path, and on the resident step forced to w-only on two workgroups (where a
    workgroup's share is under eight chunks, 45^2 and 65^2, the prefetch variant runs)."""
    from gmres_amd import _native as nat
    from tests.test_gpu_wres_carry import _workgroups_share

    _, side, kind, degree, named, N, m, params = case
    tunes = [(getattr(nat, k), v) for k, v in named]
    if route == "launch":
        tunes += [(T_RES, 0)]
    else:
        tunes += _res_tunes(12, _workgroups_share(2), 1, 0)
    c = _open(N, m, tunes, side=side, prec=(kind, degree), params=params)
    with c:
        plan = c.res_info()
        print(f"{case[0]} {route}: {plan}")
        if route == "launch":
            assert plan["variant"] is None, plan
        else:
            assert plan["variant"] == ("w-only" if N >= 130 else "prefetch") and plan["G"] == 2, plan
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, [1, 2, m], f"{case[0]} {route}", op=(side, kind, degree, params))
        prof = c.profile_read()
    if route == "launch":
        assert prof["res"][1] == 0, prof
    else:
        assert prof["res"][1] == 3 and prof["proj"][1] == 0, prof  # one resident launch per step


# ------------------------------------------------- three ranks, uneven slabs ----

@pytest.mark.parametrize("mode", ["local-launch", "xchg-res-fold1", "xchg-res-fold0"])
def test_three_rank_step(oracle, mode):
    """N = 130 over three LocalGroup ranks on one GPU (44 / 43 / 43 lines), one host thread
    per rank, each planting its slab of the same global columns: the launch path over the
    local group's collectives, and the resident step over the device exchange with the
    first dot's rank totals inside the launch (GK_TUNE_RES_FOLD 1) and by k_xchg (0)."""
    import gmres_amd as ga

    N, m, R = 130, 6, 3
    js = [1, 2, m]
    parts = ga.slab_partition(N, R)
    assert len({nl for _, nl in parts}) > 1  # uneven
    V = _V(N, m)
    g = ga.LocalGroup(R)
    ctxs = [ga.Context(N, m, device=0, line0=l0, nlines=nl) for l0, nl in parts]
    out, err, plans = [None] * R, [], [None] * R
    bar = threading.Barrier(R)
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_local(g, r, max(nl for _, nl in parts))
        if mode != "local-launch":
            for c in ctxs:
                c.xchg_local()
                c.tune(T_RES, 1)
                c.tune(T_TMO, 5000)
                c.tune(T_FOLD, 1 if mode.endswith("fold1") else 0)

        def work(r):
            try:
                c = ctxs[r]
                lo, hi = parts[r][0] * N, (parts[r][0] + parts[r][1]) * N
                c.set_precond("identity")
                c.set_rhs_ones()
                c.mgs_cycle_start()
                for k in range(m):
                    plant(c, k, V[k, lo:hi])
                plans[r] = c.res_info()
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
    print(f"{mode}: plans {plans}")
    for r in range(R):
        prof = out[r][1]
        if mode == "local-launch":
            assert plans[r]["variant"] is None and prof["res"][1] == 0 and prof["proj"][1] > 0, (plans[r], prof)
        else:
            assert plans[r]["variant"] is not None and prof["res"][1] >= len(js), (plans[r], prof)
    for i, j in enumerate(js):
        Vj, w0, ref = _ref(oracle, N, m, j)
        hs = [out[r][0][i][0] for r in range(R)]
        assert all(np.array_equal(hs[0], h) for h in hs[1:]), hs
        v = np.concatenate([out[r][0][i][1] for r in range(R)])
        check_step(hs[0], v, Vj, w0, ref, f"{mode} j={j}")


# -------------------------------- gk_update_x, gk_mgs_verr, gk_vec_* on planted columns ---

VEC_ROUTES = [("launch", 45, 12, [(T_RES, 0)]), ("resident", 130, 10, _res_tunes(2, 8, -1, -1))]  # odd and even n
_route_ids = [r[0] for r in VEC_ROUTES]


@pytest.mark.parametrize("route", VEC_ROUTES, ids=_route_ids)
def test_update_x_on_planted_columns(route):
    """x = 0; x += V y for n_out = 1 and n_out = m, against the long-double V y within
    64 eps sum_k |y_k V_k| per element; a second call accumulates."""
    _, N, m, tunes = route
    V = _V(N, m)
    ld = np.longdouble
    c = _open(N, m, tunes)
    with c:
        for n_out in (1, m):
            y = np.random.default_rng(77 + n_out).standard_normal(n_out)
            Vy = (y.astype(ld)[:, None] * V[:n_out].astype(ld)).sum(axis=0)
            mag = (np.abs(y)[:, None] * np.abs(V[:n_out])).sum(axis=0)
            c.zero_x()
            c.update_x(y)
            x1 = c.get_x()
            d1 = np.abs(x1 - Vy.astype(np.float64))
            print(f"update_x N={N} n_out={n_out}: dev/bound {np.max(d1 / (MARGIN * EPS * mag)):.3e}")
            assert np.all(d1 <= MARGIN * EPS * mag), np.nonzero(d1 > MARGIN * EPS * mag)[0][[0, -1]]
            c.update_x(y)
            x2 = c.get_x()
            d2 = np.abs(x2 - (2 * Vy).astype(np.float64))
            assert np.all(d2 <= 2 * MARGIN * EPS * mag), np.nonzero(d2 > 2 * MARGIN * EPS * mag)[0][[0, -1]]
            assert not np.array_equal(x1, x2)


def _verr_ld(V, n_out, zero_last):
    """The recurrence of gk_mgs_verr (include/gmres_hip.h; gmres_mgsr.f90:414-420) in long
    double on the Gram matrix of rows 0..n_out."""
    ld = np.longdouble
    Vl = V[: n_out + 1].astype(ld)
    G = Vl @ Vl.T
    if zero_last:
        G[n_out, :] = 0
        G[:, n_out] = 0
    v = np.zeros(n_out + 1, dtype=ld)
    for j in range(1, n_out + 1):
        s = ld(0)
        for i in range(1, j + 1):
            s += 2 * G[j, i - 1] ** 2
        s += (G[j, j] - 1) ** 2
        v[j] = np.sqrt(v[j - 1] ** 2 + s)
    return v.astype(np.float64)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("route", VEC_ROUTES, ids=_route_ids)
def test_mgs_verr_on_planted_columns(route, order):
    """Gram entries ~1e-5 instead of rounding noise: v_err to 1e-10 relative, in the
    reference's dot order (GK_TUNE_VERR_ORDER 1) and tree-reduced (0), with and without the
    zeroed last column."""
    from gmres_amd import _native as nat

    _, N, m, tunes = route
    V = _V(N, m)
    c = _open(N, m, tunes + [(T_VERR_ORDER, order)])
    with c:
        for zero_last in (0, 1):
            n_out = m - 1
            ve = np.zeros(m + 1)
            nat.check(nat.hip().gk_mgs_verr(c.handle, n_out, zero_last, ve.ctypes.data_as(nat._dp)), "gk_mgs_verr")
            ref = _verr_ld(V, n_out, zero_last)
            assert ref[1] > 1e-8  # Gram terms ~pert / N: signal, not noise
            print(f"verr N={N} order={order} zero_last={zero_last}: max rel dev "
                  f"{np.max(np.abs(ve[1:n_out + 1] - ref[1:]) / ref[1:]):.3e}")
            assert ve[0] == 0.0
            assert np.allclose(ve[1: n_out + 1], ref[1:], rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("route", VEC_ROUTES, ids=_route_ids)
def test_vec_dot_and_lincomb_on_planted_columns(route):
    """gk_vec_dot within the dot bound; the gk_vec_lincomb forms are element-wise and the
    library is built without FMA contraction, so they equal the float64 expression in the
    header's association exactly -- with out aliasing a and with out distinct."""
    from gmres_amd import _native as nat

    _, N, m, tunes = route
    L = nat.hip()
    V = _V(N, m)
    ld = np.longdouble
    s1, s2 = 0.7310585786300049, -1.6180339887498949
    A, B, C, OUT = 2 + 0, 2 + 1, 2 + 2, 2 + m  # columns 0, 1, 2 and the free column m
    a, b, cc = V[0], V[1], V[2]
    forms = {1: a + s1 * b, 2: (a + s1 * b) + s2 * cc, 3: a + s1 * (b - s2 * cc), 4: np.zeros_like(a)}
    c = _open(N, m, tunes)
    with c:
        d = ctypes.c_double()
        for (i, k) in ((0, 1), (2, 2), (m - 1, 0)):
            nat.check(L.gk_vec_dot(c.handle, 2 + i, 2 + k, ctypes.byref(d)), "gk_vec_dot")
            ref = float(np.dot(V[i].astype(ld), V[k].astype(ld)))
            bound = MARGIN * EPS * np.linalg.norm(V[i]) * np.linalg.norm(V[k])
            print(f"vec_dot N={N} ({i},{k}): dev/bound {abs(d.value - ref) / bound:.3e}")
            assert abs(d.value - ref) <= bound
        for form, want in forms.items():
            for alias in (False, True):
                out = A if alias else OUT
                nat.check(L.gk_vec_lincomb(c.handle, form, out, A, B, C, s1, s2), "gk_vec_lincomb")
                c.sync()
                got = read_col(c, out - 2)
                assert np.array_equal(got, want), (form, alias, np.nonzero(got != want)[0][[0, -1]])
                if alias:
                    plant(c, 0, a)
                else:  # the inputs are untouched
                    assert np.array_equal(read_col(c, 0), a) and np.array_equal(read_col(c, 1), b)
