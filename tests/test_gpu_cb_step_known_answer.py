"""One Arnoldi step of the FP32-compressed basis (gk_set_basis_precision GK_BASIS_F32,
gmres_amd/csrc/gk_cb.hip) on planted, asymmetric float columns against a long-double step
(tests/general_data.py).

tests/test_gpu_cb.py feeds b = A*1 throughout and compares the two device routes with each
other or with a restatement at 1e-9; both routes share cb_round, the float columns and vjw.
Here a context's cycle is opened, float columns 0..j-1 are overwritten through gk_set_basis
with planted_basis rounded once to float32 (column j-1 last: it is the operator's input),
step j runs, and the step is held to

    |h_i - h_ref_i|         <= 64 eps ||w0|| ||V_i||          (||V_i|| = 1 for h_{j+1})
    stored_e                 = its own float32 round trip
    |stored_e - v_ref_e|    <= ulp32(v_ref_e) / 2 + 64 eps max |v_ref|      for EVERY element
    vjw (vector id m + 2)    = the stored column widened, bit for bit

with (h_ref, v_ref) = cb_step_ld(V, w0) -- v_ref unrounded, in long double -- and w0 the
oracle's operator on the widened column j-1 (bit-exact with the device operators).  The
column criterion says: the stored value is a correct round-to-nearest of some value within
the FP64 step bound of the reference.  A truncating conversion, a division in float or h
rounded to float first exceed it by 6e4 or more and move no h (tests/test_cb_step_data.py,
which pins every (N, m, j) and operator used here on the CPU).

The preconditioned cases take the step's first dot <w, V(:,1)> from the operator launch's
epilogue (its partner read from v1w); test_gpu_step_known_answer.py runs the same cases on
the FP64 basis.  The same planted contexts check gk_update_x, gk_mgs_verr and gk_set_basis
itself.
"""
import numpy as np
import pytest

from tests import verr_host
from tests.general_data import (CB_LAUNCH_SHAPES, PREC_STEP_CASES, CB_RES_JS, CB_RES_M, CB_RES_PLANS, EPS, MARGIN, PARAMS,
                                cb_planted, cb_step_ld, check_cb_step, op_w0, planted_basis_f32)

pytestmark = pytest.mark.gpu

T_PROJ_NT, T_PROJ_BLOCKS, T_RES, T_SHARE, T_TMO, T_VERR_ORDER, T_GRAPH = 0, 1, 8, 10, 11, 14, 19

_refs: dict = {}


def _ref(oracle, N, m, j, side="left", prec="identity", degree=1, params=PARAMS):
    """(V[:j], w0, (h_ref, v_ref in long double)) of step j on the planted float columns."""
    key = (N, m, j, side, prec, degree, params)
    if key not in _refs:
        V = cb_planted(N, m)[:j]
        w0 = op_w0(oracle, V[j - 1], N, side, prec, degree, params)
        _refs[key] = (V, w0, cb_step_ld(V, w0))
    return _refs[key]


def _tunes(named):
    from gmres_amd import _native as nat

    return [(getattr(nat, k) if isinstance(k, str) else k, v) for k, v in named]


def _open(N, m, tunes, side="left", prec="identity", degree=1, ncols=None, params=PARAMS):
    """An FP32-basis context with its tuning applied and an MGS-R cycle open; columns
    0..ncols-1 (default m) planted through gk_set_basis."""
    import gmres_amd as ga

    c = ga.Context(N, m)
    try:
        for k, v in _tunes(tunes):
            c.tune(k, v)
        c.set_precond(prec, params, degree, side=side)
        c.set_basis("f32")
        c.set_rhs_ones()
        c.mgs_cycle_start()
        ncols = m if ncols is None else ncols
        V = cb_planted(N, max(m, ncols))
        for k in range(ncols):
            c.put_basis(k, V[k])
    except Exception:
        c.close()
        raise
    return c


def _read_vjw(c):
    """The operator's input vector (vector id m + 2) through x."""
    from gmres_amd import _native as nat

    nat.check(nat.hip().gk_vec_lincomb(c.handle, 0, 0, c.m + 2, 0, 0, 0.0, 0.0), "gk_vec_lincomb")  # GK_LC_COPY
    return c.get_x()


def _step(c, N, m, j):
    """Step j on the planted columns: column j-1 planted last (the operator's input), the
    output column planted again afterwards so that a later step sees the planted set."""
    V = cb_planted(N, m)
    c.put_basis(j - 1, V[j - 1])
    h = c.mgs_step(j)
    v = c.get_basis(j)
    vjw = _read_vjw(c)
    if j < m:
        c.put_basis(j, V[j])
    return h, v, vjw


def _check(oracle, c, N, m, js, what, twice=False, op=("left", "identity", 1)):
    worst = [0.0, -np.inf, 0]
    plan = c.res_info()
    for j in js:
        V, w0, ref = _ref(oracle, N, m, j, *op)
        for rep in range(2 if twice else 1):
            h, v, vjw = _step(c, N, m, j)
            tag = f"{what} N={N} m={m} j={j}" + (" (replay)" if rep else "")
            r = check_cb_step(h, v, V, w0, ref, tag, plan=plan)
            assert np.array_equal(vjw, v), f"{tag}: vjw differs from the stored column at {np.nonzero(vjw != v)[0][[0, -1]]}"
            worst = [max(worst[0], r[0]), max(worst[1], r[1]), worst[2] + r[2]]
    print(f"{what} N={N} m={m}: worst h dev/bound {worst[0]:.3e}, column excess/vb {worst[1]:.3e}, "
          f"{worst[2]} elements off float32(v_ref)")
    return worst


# ---------------------------------------------------------------- launch path ---

LAUNCH_CASES = ([(N, m, 0, nt) for N, m in CB_LAUNCH_SHAPES for nt in (1, 0)]
                + [(N, m, 3, nt) for N, m in CB_LAUNCH_SHAPES if N >= 45 for nt in (1, 0)])


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("N,m,blocks,nt", LAUNCH_CASES)
def test_launch_path_step(oracle, N, m, blocks, nt, graph):
    """k_proj<..., float> / k_scale_cb (GK_TUNE_RES 0), call by call and as a hipGraph (every graph step
    twice: the second is a replay), non-temporal column loads and not; j = 1, 2, m.
    GK_TUNE_PROJ_BLOCKS 3: at 130^2 the U = 2 form, six trips of the grid-stride loop with a
    ragged last one; at 45^2 (1012 double2: any block count leaves at most four per thread) the
    U = 4 form on three workgroups, its one trip ragged.  The default is U = 4, one trip."""
    tunes = [(T_RES, 0), (T_GRAPH, graph), (T_PROJ_NT, nt)] + ([(T_PROJ_BLOCKS, blocks)] if blocks else [])
    c = _open(N, m, tunes)
    with c:
        assert c.res_info()["variant"] is None
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, [1, 2, m], f"launch graph={graph} blocks={blocks} nt={nt}", twice=bool(graph))
        prof = c.profile_read()
    assert prof["res"][1] == 0, prof
    if graph:
        assert prof["graph"][1] > 0, prof
    else:
        assert prof["graph"][1] == 0 and prof["proj"][1] > 0, prof


# ------------------------------------------------------------------- resident ---

def _share(wg):
    """(GK_TUNE_RES_SHARE leaving wg workgroups, the device's CUs)."""
    from tests import test_gpu_wres_carry as tw

    s = tw._workgroups_share(wg)
    return s, tw._cus[0]


@pytest.mark.parametrize("N,wg,r2e,l2e,stream2,odd", CB_RES_PLANS)
def test_resident_step(oracle, N, wg, r2e, l2e, stream2, odd):
    """k_mgs_wcb on the plans of general_data.CB_RES_PLANS: a single unpaired chunk; pair +
    single; odd counts, a clipped last workgroup with an even count of its own and workgroups
    with nothing (130^2 on 1 / 2 / 4 / 16); every part at once (259^2: LDS pairs + single, the
    two-deep streamed loop with a ragged second trip, the tail); LDS on two workgroups with
    the streamed part owned by one (309^2); LDS pairs only (320^2); full even register ranges
    (512^2 on 8).  j = 1, 2, 5, m; one resident launch per step, no projection launch."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    m, n = CB_RES_M, N * N
    share, cus = _share(wg)
    c = _open(N, m, [(T_RES, 1), (T_SHARE, share), (T_TMO, 5000)])
    with c:
        plan = c.res_info()
        q = ga.cb_plan_query(n, cus=cus, share=share, m=m)
        print(f"resident N={N} on {wg} workgroups: {plan}")
        assert plan["variant"] == nat.RES_VARIANTS[nat.GK_RES_CB], plan
        assert (plan["G"], plan["r2e"], plan["l2e"], plan["nres2"]) == (q["G"], q["r2e"], q["l2e"], q["nres2"]), (plan, q)
        assert (plan["G"], plan["r2e"], plan["l2e"], n // 2 - plan["nres2"], bool(n & 1)) == (wg, r2e, l2e, stream2, odd), plan
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, list(CB_RES_JS), f"resident wg={wg}")
        prof = c.profile_read()
    assert prof["res"][1] == len(CB_RES_JS) and prof["proj"][1] == 0, prof


# ----------------------------- the first dot from the operator launch's epilogue ---

@pytest.mark.parametrize("route", ["launch", "resident"])
@pytest.mark.parametrize("case", PREC_STEP_CASES, ids=[c[0] for c in PREC_STEP_CASES])
def test_preconditioned_step(oracle, case, route):
    """Left cbpr2 and Chebyshev (one fused pass over several windows, two passes, per-sweep
    kernels; the stencil as stage 0 of the pass and as a launch of its own), right cbpr2
    (the fused march and two launches) and Chebyshev(3): <w, V(:,1)> comes from the operator
    launch's epilogue, its partner from v1w.  j = 1, 2, m on the launch path; the resident
    route on two workgroups (130^2: 17 + 16 chunks)."""
    from gmres_amd import _native as nat

    _, side, prec, degree, named, N, m, params = case
    if route == "launch":
        tunes = [(T_RES, 0)] + list(named)
    else:
        tunes = [(T_RES, 1), (T_SHARE, _share(2)[0]), (T_TMO, 5000)] + list(named)
    c = _open(N, m, tunes, side=side, prec=prec, degree=degree, params=params)
    with c:
        plan = c.res_info()
        if route == "launch":
            assert plan["variant"] is None, plan
        else:
            assert plan["variant"] == nat.RES_VARIANTS[nat.GK_RES_CB] and plan["G"] == 2, plan
            if N == 130:
                assert plan["r2e"] == 17 and plan["l2e"] == 0, plan
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, [1, 2, m], f"{case[0]} {route}", op=(side, prec, degree, params))
        prof = c.profile_read()
    if route == "launch":
        assert prof["res"][1] == 0, prof
    else:
        assert prof["res"][1] == 3 and prof["proj"][1] == 0, prof


# ------------------------------------------------------ the float-column readers ---

VEC_ROUTES = [("launch-45", 45, 12, [(T_RES, 0)]), ("resident-130", 130, 10, [(T_RES, 1), (T_TMO, 5000)])]  # odd, even n


UPDATE_OPS = [("left", "identity"), ("right", "identity"), ("right", "cbpr2")]


@pytest.mark.parametrize("side,prec", UPDATE_OPS, ids=[f"{s}-{p}" for s, p in UPDATE_OPS])
@pytest.mark.parametrize("route", VEC_ROUTES, ids=[r[0] for r in VEC_ROUTES])
def test_update_x_on_planted_columns(oracle, route, side, prec):
    """gk_update_x for n_out = 1 and n_out = m against the long-double evaluation on the
    widened columns: into x = 0, then -- with another y -- into a random non-zero x planted
    through set_x, which separates the accumulator from the product.

    Left, and right with the identity (right_prec is false there: the same launch as left):
    k_update_x<ADD, float> forms x + V y; the bound is 64 eps sum_k |y_k V_k| =: 64 eps mag per
    element, and the planted x is u mag with |u| <= 1, so that the closing addition rounds
    within eps mag and the bound needs no term of its own for x.

    Right with cbpr2: the other form, k_update_x<false, float> writes t = V y into w, then
    x += M^-1 t (cbpr2 sweep + k_add; the profile must show the sweep and two update launches
    per call).  w has no vector id, so x is held, against x + M^-1 (V y) with
    cbpr2 in long double.  Bound: 64 eps |M^-1| mag with |M^-1| u = u / d + |alpha| (u + |A| u / d)
    taken term by term as cbpr2 evaluates it (general_data.cbpr2_abs), the planted x again
    within it.  To first order the error is at most (n_out + 1) eps mag in t, carried through
    M^-1, plus ~8 roundings of the sweep and 2 of the addition, each within eps |M^-1| mag:
    (n_out + 11) eps |M^-1| mag <= 23 eps |M^-1| mag at n_out = 12."""
    from tests.general_data import cbpr2_abs, cbpr2_ld

    _, N, m, tunes = route
    V = cb_planted(N, m)
    ld = np.longdouble
    right = side == "right" and prec != "identity"
    c = _open(N, m, tunes, side=side, prec=prec)
    with c:
        c.profile(True)
        c.profile_reset()
        for n_out in (1, m):
            for call, seed in enumerate((77 + n_out, 977 + n_out)):
                rng = np.random.default_rng(seed)
                y = rng.standard_normal(n_out)
                Vy = (y.astype(ld)[:, None] * V[:n_out].astype(ld)).sum(axis=0)
                mag = (np.abs(y)[:, None] * np.abs(V[:n_out])).sum(axis=0)
                if right:
                    Vy, mag = cbpr2_ld(oracle, Vy, N), cbpr2_abs(oracle, mag, N)
                x0 = rng.uniform(-1.0, 1.0, N * N) * mag if call else np.zeros(N * N)
                assert call == 0 or np.max(np.abs(x0)) > 0.5 * np.max(mag)
                c.set_x(x0)
                c.update_x(y)
                x = c.get_x()
                d = np.abs(x.astype(ld) - (x0.astype(ld) + Vy)).astype(np.float64)
                print(f"update_x N={N} {side} {prec} n_out={n_out} into {'a planted' if call else 'zero'} x: "
                      f"dev/bound {np.max(d / (MARGIN * EPS * mag)):.3e}")
                assert np.all(d <= MARGIN * EPS * mag), np.nonzero(d > MARGIN * EPS * mag)[0][[0, -1]]
                assert not np.array_equal(x, x0)
        prof = c.profile_read()
    print(f"update_x N={N} {side} {prec}: update launches {prof['update'][1]}, cbpr2 sweeps {prof['stencil'][1]}")
    if right:  # per call: k_update_x<false, float>, the cbpr2 sweep (profiled with the stencil launches), k_add
        assert prof["update"][1] == 8 and prof["stencil"][1] == 4, prof
    else:
        assert prof["update"][1] == 4 and prof["stencil"][1] == 0, prof


def _verr(c, n_out, zero_last):
    from gmres_amd import _native as nat

    ve = np.zeros(c.m + 1)
    nat.check(nat.hip().gk_mgs_verr(c.handle, n_out, zero_last, ve.ctypes.data_as(nat._dp)), "gk_mgs_verr")
    return ve


def _verr_ref(V, n_out, zero_last):
    """verr_host.mgs_verr with exact_dot; zero_last: the last column's Gram row and column 0."""
    cols = [v for v in V[: n_out + 1]]
    if zero_last:
        cols[n_out] = np.zeros_like(cols[n_out])
    return verr_host.mgs_verr(cols, n_out, verr_host.exact_dot)[: n_out + 1]


@pytest.mark.parametrize("route", VEC_ROUTES, ids=[r[0] for r in VEC_ROUTES])
def test_mgs_verr_on_planted_columns(route):
    """k_gram<float> on Gram entries ~1e-5: v_err to 1e-10 relative of the exact-dot evaluation,
    with and without the zeroed last column; GK_TUNE_VERR_ORDER 1 and 0 give the same bits
    (the float route is the tree either way)."""
    _, N, m, tunes = route
    V = cb_planted(N, m)
    got = {}
    for order in (1, 0):
        c = _open(N, m, tunes + [(T_VERR_ORDER, order)])
        with c:
            for zero_last in (0, 1):
                n_out = m - 1
                ve = _verr(c, n_out, zero_last)
                ref = _verr_ref(V, n_out, zero_last)
                assert ref[1] > 1e-8  # Gram terms ~pert / N: signal, not noise
                print(f"verr N={N} order={order} zero_last={zero_last}: max rel dev "
                      f"{np.max(np.abs(ve[1:n_out + 1] - ref[1:]) / ref[1:]):.3e}")
                assert ve[0] == 0.0
                assert np.allclose(ve[1: n_out + 1], ref[1:], rtol=1e-10, atol=0.0)
                got[(order, zero_last)] = ve
    for zero_last in (0, 1):
        assert np.array_equal(got[(1, zero_last)], got[(0, zero_last)])


def test_mgs_verr_at_the_column_limit():
    """n_out + 1 = 128 columns (GCMAX: every pair slot of k_gram<float>'s tile) at 45^2, and
    129 columns, which must be refused (GK_ERR_ARG) before anything is launched."""
    from gmres_amd import _native as nat

    N = 45
    V = cb_planted(N, 128)
    c = _open(N, 127, [(T_RES, 0)], ncols=128)
    with c:
        ve = _verr(c, 127, 0)
        ref = _verr_ref(V, 127, 0)
        print(f"verr N={N} 128 columns: max rel dev {np.max(np.abs(ve[1:] - ref[1:]) / ref[1:]):.3e}")
        assert np.allclose(ve[1:], ref[1:], rtol=1e-10, atol=0.0)
    c = _open(N, 128, [(T_RES, 0)], ncols=3)
    with c:
        c.profile(True)
        c.profile_reset()
        ve = np.zeros(130)
        assert nat.hip().gk_mgs_verr(c.handle, 128, 0, ve.ctypes.data_as(nat._dp)) == nat.GK_ERR_ARG
        assert "128" in nat.last_error()
        assert c.profile_read()["other"][1] == 0


# ---------------------------------------------------------------- gk_set_basis ---

@pytest.mark.parametrize("basis", ["f64", "f32"])
def test_put_basis_round_trip(basis):
    """gk_set_basis then gk_get_basis, bit for bit, at odd n on every column 0..m; on the
    FP32 basis a value that is no float is refused and the column is unchanged, and vjw /
    v1w hold what was planted."""
    import gmres_amd as ga
    from gmres_amd import _native as nat

    N, m = 45, 5
    rng = np.random.default_rng(11)
    with ga.Context(N, m) as c:
        c.set_basis(basis)
        c.set_rhs_ones()
        c.mgs_cycle_start()
        cols = [rng.standard_normal(N * N) for _ in range(m + 1)]
        if basis == "f32":
            cols = [v.astype(np.float32).astype(np.float64) for v in cols]
        for k in (0, 1, 2, 3, 4, 5):
            c.put_basis(k, cols[k])
        for k in range(m + 1):
            assert np.array_equal(c.get_basis(k), cols[k]), k
        assert c.mgs_step(1).size == 2  # the cycle is still open
        L = nat.hip()
        bad = np.zeros(N * N)
        assert L.gk_set_basis(c.handle, -1, bad.ctypes.data_as(nat._dp)) == nat.GK_ERR_ARG
        assert L.gk_set_basis(c.handle, m + 1, bad.ctypes.data_as(nat._dp)) == nat.GK_ERR_ARG
        if basis == "f32":
            c.put_basis(3, cols[3])
            assert np.array_equal(_read_vjw(c), cols[3])
            c.put_basis(0, cols[0])
            nat.check(L.gk_vec_lincomb(c.handle, 0, 0, m + 1, 0, 0, 0.0, 0.0), "gk_vec_lincomb")  # v1w -> x
            assert np.array_equal(c.get_x(), cols[0]) and np.array_equal(_read_vjw(c), cols[0])
            bad = cols[2].copy()
            bad[-1] = 1.0 + 2.0 ** -30  # the odd tail element; not a float
            assert L.gk_set_basis(c.handle, 2, bad.ctypes.data_as(nat._dp)) == nat.GK_ERR_ARG
            assert "FP32" in nat.last_error()
            assert np.array_equal(c.get_basis(2), cols[2])
            assert np.array_equal(_read_vjw(c), cols[0])
        else:
            bad = cols[2].copy()
            bad[-1] = 1.0 + 2.0 ** -30
            c.put_basis(2, bad)
            assert np.array_equal(c.get_basis(2), bad)


def test_put_basis_ends_a_short_recurrence_solve():
    import gmres_amd as ga

    with ga.Context(32, 8) as c:
        c.set_rhs_ones()
        s = ga.SrSolve(c, "pcg", 0.0, 20)
        s.iterate(5)
        s.status()
        c.put_basis(0, np.zeros(32 * 32))
        with pytest.raises(ga.GkError):
            s.iterate(1)
        with pytest.raises(ga.GkError):
            s.status()


def test_planted_columns_are_what_the_reference_consumes():
    """The device holds exactly planted_basis_f32: the reference and the step see one set."""
    N, m = 45, 8
    V32 = planted_basis_f32(N, m, seed=7000 + 7 * N + m)
    c = _open(N, m, [(T_RES, 0)])
    with c:
        for k in range(m):
            assert np.array_equal(c.get_basis(k).astype(np.float32), V32[k])
