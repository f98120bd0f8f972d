"""One Householder step on planted reflectors against a long-double step
(tests/hh_data.py).

Every other Householder check is a residual history held to the tiers 1e-8 / 1e-3 / 5e-2, or
gk_hh_verr fed the device's own reflectors; GMRES corrects a slightly wrong H at the next
restart, so none of them sees a step that is wrong in its last ten digits.  Here a context's
Householder cycle is opened, the reflector columns P_1..P_m are overwritten with planted ones
(hh_data.planted_reflectors: unit rows, zero below their pivot, pivot^2 in [0.5, 0.9), Gaussian
tails -- v_j = P_1..P_j e_j is dense and has none of the square's symmetries), gk_hh_step(j)
runs, and its Hessenberg column and new reflector are held to hh_data.hh_step_ld:

    |h_i - h_ref_i|                <= 64 eps ||w0||           i = 0..j
    |p[j] - p_ref[j]|              <= 64 eps |p_ref[j]|       the pivot, 0.7 .. 1
    max |p[j+1:] - p_ref[j+1:]|    <= 64 eps max |p_ref[j+1:]|  the rest, ~1/N
    p[:j] == 0 exactly

tests/test_hh_data.py pins on the CPU, for every (N, m, j) run here, that a float64 step
with another summation tree stays below 1/8 of each bound and that a tail norm started one
element early or late, a fix-up one element off, the last element of P_j not read, the
DOWN chain's leading dot taken one element off and a skipped 512-element chunk each exceed
one.  The sign of h[j] follows w_j before the fix-up; hh_data.hh_reference asserts that it is
2^20 h-bounds away from zero.

A step reads every reflector from HBM and writes column j (P_{j+1}), which is planted again
before the next step.  gk_hh_update_x and the basis gk_hh_verr rebuilds are checked on the
same planted contexts.
"""
import threading

import numpy as np
import pytest

from tests import hh_data as hd
from tests import test_gpu_resident as tr
from tests.general_data import plant

pytestmark = pytest.mark.gpu

T_RES, T_R2, T_SHARE, T_TMO, T_WONLY, T_VERR_ORDER, T_HH_FUSE, T_PC, T_FOLD, T_HH_NORM_ORDER = (8, 9, 10, 11, 13, 14, 15, 21,
                                                                                                22, 25)


def _res_tunes(r2, share, wonly, pc):
    return [(T_PC, pc), (T_RES, 1), (T_WONLY, wonly), (T_R2, r2), (T_SHARE, share), (T_TMO, 5000)]


def _step(c, N, m, j, precondition=False, split=False):
    """Step j on the planted reflectors; its output column is then planted again."""
    h, p = hd.hh_dev_step(c, j, precondition, split)
    if j < m:
        plant(c, j, hd.reflectors(N, m)[j])
    return h, p


def _check(oracle, c, N, m, js, what, precondition=False):
    worst = (0.0, 0.0, 0.0)
    plan = c.res_info(hh=True)
    for j in js:
        ref = hd.reference(oracle, N, m, j, precondition)
        h, p = _step(c, N, m, j, precondition)
        r = hd.check_hh_step(h, p, ref, j, f"{what} N={N} m={m} j={j}", plan=plan)
        worst = tuple(max(a, b) for a, b in zip(worst, r))
    print(f"{what} N={N} m={m}: worst dev/bound h {worst[0]:.3e}, pivot {worst[1]:.3e}, rest {worst[2]:.3e}")
    return worst


# ---------------------------------------------------------------- launch path ---

@pytest.mark.parametrize("N,m", hd.LAUNCH_SHAPES)
def test_launch_path_step(oracle, N, m):
    """k_set_unit, the PJ_AXPY_DOT chains with coefficient 2, PJ_AXPY_NORM with its tail
    offset, k_hh_pivot, k_hh_fix and k_scale (GK_TUNE_RES 0).  (2, 3) with j = 3 puts the tail
    on the last element of the vector; (3, 5) and (45, 12) are odd n."""
    c = hd.hh_open(N, m, [(T_RES, 0)])
    with c:
        assert c.res_info(hh=True)["variant"] is None
        c.profile(True)
        c.profile_reset()
        _check(oracle, c, N, m, hd.launch_js(m), "hh launch")
        prof = c.profile_read()
    assert prof["res"][1] == 0 and prof["proj"][1] > 0, prof


def test_async_then_wait_is_the_step():
    N, m, j = 45, 12, 5
    c = hd.hh_open(N, m, [(T_RES, 0)])
    with c:
        h1, p1 = _step(c, N, m, j)
        h2, p2 = _step(c, N, m, j, split=True)
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)


def test_sequential_norms_step(oracle):
    """GK_TUNE_HH_NORM_ORDER 1: the reflector norms as one running sum (one rank, unfused);
    test_hh_data.py::test_hh_sequential_norms_pin is its CPU pin."""
    N, m = 45, 12
    c = hd.hh_open(N, m, [(T_RES, 0), (T_HH_NORM_ORDER, 1)])
    with c:
        _check(oracle, c, N, m, hd.launch_js(m), "hh launch, sequential norms")


# ------------------------------------------------------------ resident chains ---

RES_CASES = ([(N, m, r2, share, wonly, -1, f, "w-only" if wonly == 1 else "any")
              for N, m, _, r2, share, wonly in tr.HCASES for f in ((1, 0) if wonly == 1 else (1,))]
             + [(N, m, r2, share, wonly, 1, 1, "w+column") for N, m, _, r2, share, wonly in tr.HPCASES]
             # the w-only chains' LDS part and a long streamed part, which none of HCASES reaches
             + [c + (-1, f, "w-only+lds") for c in hd.WONLY_LDS_CASES for f in (1, 0)])


@pytest.mark.parametrize("N,m,r2,share,wonly,pc,fuse,variant", RES_CASES)
def test_resident_step(oracle, N, m, r2, share, wonly, pc, fuse, variant):
    """RES_HH_DOWN with the unit vector known (and built in the launch when fused), RES_HH_UP
    with its tail norm, and the w-only variant's fused close (GK_TUNE_HH_FUSE 1: zeroing,
    fix-up, hb and the renormalisation inside the launch) against 0: the forcing tuples of
    test_gpu_resident.HCASES / HPCASES, j = 1, 2, 5 and m.  Fused and unfused are each held to
    the long-double step, not to each other."""
    c = hd.hh_open(N, m, _res_tunes(r2, share, wonly, pc) + [(T_HH_FUSE, fuse)])
    with c:
        plan = c.res_info(hh=True)
        print(f"hh resident N={N} m={m} r2={r2} share={share} wonly={wonly} pc={pc} fuse={fuse}: {plan}")
        if variant == "any":
            assert plan["variant"] is not None, plan
        elif variant == "w-only+lds":  # registers, LDS and a streamed part (odd N: and the last element)
            assert plan["variant"] == "w-only" and plan["r2e"] == 90 and plan["l2e"] > 0 and 2 * plan["nres2"] < N * N - 1, plan
        else:
            assert plan["variant"] == variant, plan
        c.profile(True)
        c.profile_reset()
        js = hd.resident_js(m)
        _check(oracle, c, N, m, js, f"hh resident {plan['variant']} fuse={fuse}")
        prof = c.profile_read()
    assert prof["res"][1] >= len(js) and prof["proj"][1] == 0, prof  # no k_proj launch stood in for a chain


# ------------------------------------------------------- preconditioned step ---

@pytest.mark.parametrize("N,m,tunes,variant", [(45, 12, [(T_RES, 0)], None),
                                               (181, 16, _res_tunes(12, 128, 1, -1) + [(T_HH_FUSE, 1)], "w-only")],
                         ids=["launch", "w-only-fused"])
def test_preconditioned_step(oracle, N, m, tunes, variant):
    """precondition = 1 with cbpr2 on the left: w0 = cbpr2(A v).  The oracle's operator and
    cbpr2 are bit-exact with the device on equal input; the reference applies them to its own
    v rounded to float64 (test_hh_data.py::test_hh_preconditioned_step_pin)."""
    assert (N, m) in hd.PREC_SHAPES
    c = hd.hh_open(N, m, tunes, precondition=True)
    with c:
        assert c.res_info(hh=True)["variant"] == variant
        js = hd.launch_js(m) if variant is None else hd.resident_js(m)
        _check(oracle, c, N, m, js, f"hh cbpr2 {variant or 'launch'}", precondition=True)


# ------------------------------------------------- three ranks, uneven slabs ----

@pytest.mark.parametrize("mode", ["local-launch", "xchg-res-fold1", "xchg-res-fold0"])
def test_three_rank_step(oracle, mode):
    """N = 130 over three LocalGroup ranks on one GPU (44 / 43 / 43 lines), one host thread per
    rank, each planting its slab of the same global reflectors: hh_pivot's broadcast from the
    owner of index j (rank 0; the tail offset j - g0 is negative on the others), the launch
    path over the local group's collectives and the resident chains over the device exchange
    with the first dot's rank totals inside the launch (GK_TUNE_RES_FOLD 1) and by k_xchg (0)."""
    import gmres_amd as ga

    N, m, R = 130, 6, 3
    js = [1, 2, m]
    parts = ga.slab_partition(N, R)
    assert len({nl for _, nl in parts}) > 1 and parts[0][1] * N > m + 2  # uneven; rank 0 owns every pivot
    P = hd.reflectors(N, m)
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
                hd.hh_start(c, P[:, lo:hi])
                plans[r] = c.res_info(hh=True)
                c.profile(True)
                c.profile_reset()
                res = []
                for j in js:
                    bar.wait(timeout=60)  # every rank's reflectors are in place
                    h, p = hd.hh_dev_step(c, j)
                    bar.wait(timeout=60)  # every rank has read before anyone re-plants
                    if j < m:
                        plant(c, j, P[j, lo:hi])
                    res.append((h, p))
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
    print(f"hh {mode}: plans {plans}")
    for r in range(R):
        prof = out[r][1]
        if mode == "local-launch":
            assert plans[r]["variant"] is None and prof["res"][1] == 0 and prof["proj"][1] > 0, (plans[r], prof)
        else:
            assert plans[r]["variant"] is not None and prof["res"][1] >= len(js) and prof["proj"][1] == 0, (plans[r], prof)
    worst = (0.0, 0.0, 0.0)
    for i, j in enumerate(js):
        ref = hd.reference(oracle, N, m, j)
        hs = [out[r][0][i][0] for r in range(R)]
        assert all(np.array_equal(hs[0], h) for h in hs[1:]), hs
        p = np.concatenate([out[r][0][i][1] for r in range(R)])
        worst = tuple(max(a, b) for a, b in zip(worst, hd.check_hh_step(hs[0], p, ref, j, f"hh {mode} j={j}")))
    print(f"hh three ranks {mode}: worst dev/bound h {worst[0]:.3e}, pivot {worst[1]:.3e}, rest {worst[2]:.3e}")


# -------------------------- gk_hh_update_x and gk_hh_verr's rebuilt basis ---

VEC_ROUTES = [("launch", 45, 12, [(T_RES, 0)]), ("w-only", 181, 16, _res_tunes(12, 128, 1, -1))]
_route_ids = [r[0] for r in VEC_ROUTES]


@pytest.mark.parametrize("route", VEC_ROUTES, ids=_route_ids)
def test_update_x_on_planted_reflectors(route):
    """x + P_1..P_m [y; 0] (k_set_prefix, the DOWN chain without a unit vector, k_add) for a
    seeded asymmetric x and a seeded y of length n_out = m, within 64 eps (max|x| + ||y||) per
    element of the long-double evaluation."""
    from gmres_amd import _native as nat

    name, N, m, tunes = route
    assert (N, m) in hd.VEC_SHAPES
    x, y = hd.vec_data(N, m)
    ref = hd.update_x_ld(hd.reflectors(N, m), x, y).astype(np.float64)
    c = hd.hh_open(N, m, tunes)
    with c:
        plan = c.res_info(hh=True)
        assert (plan["variant"] is None) == (name == "launch") and name in ("launch", plan["variant"]), plan
        c.set_x(x)
        nat.check(nat.hip().gk_hh_update_x(c.handle, y.ctypes.data_as(nat._dp), m), "gk_hh_update_x")
        got = c.get_x()
    d, b = np.abs(got - ref), hd.update_x_bound(x, y)
    print(f"hh update_x {name} N={N} m={m}: dev/bound {d.max() / b:.3e}")
    bad = np.nonzero(~(d <= b))[0]
    assert bad.size == 0, f"x off at {bad.size} elements, first {bad[0]}, last {bad[-1]}, max dev {d.max():.3e} bound {b:.3e}"


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("route", VEC_ROUTES, ids=_route_ids)
def test_verr_rebuilt_basis_on_planted_reflectors(route, order):
    """Column k of the basis gk_hh_verr rebuilds against P_1..P_k e_k in long double, every
    k = 1..m: within 64 eps max|v_ref| per element, and with the tree-reduced chains
    (GK_TUNE_VERR_ORDER 0: the DOWN chains of the route, unit vector known) also within
    64 eps max|v_ref off index k-1| off the column's own entry 1 - 2 P_k(k)^2, which stands
    over a bulk of ~1/N.  The reference-order rebuild (1, the default: k_hh_rebuild_dot / _upd,
    one running sum per dot) meets only the first on the CPU (test_hh_data.py)."""
    from gmres_amd import _native as nat

    name, N, m, tunes = route
    P = hd.reflectors(N, m)
    c = hd.hh_open(N, m, tunes + [(T_VERR_ORDER, order)])
    with c:
        ve = np.zeros(m + 1)
        nat.check(nat.hip().gk_hh_verr(c.handle, m, ve.ctypes.data_as(nat._dp)), "gk_hh_verr")
        cols = [c.get_basis(k, 1) for k in range(m)]
    worst = (0.0, 0.0)
    for k in range(1, m + 1):
        r = hd.rebuilt_ratios(cols[k - 1], hd.rebuilt_ld(P, k), k)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        assert r[0] <= 1.0 and (order == 1 or r[1] <= 1.0), (k, r)
    print(f"hh rebuilt basis {name} order={order} N={N} m={m}: worst dev/bound {worst[0]:.3e}, off the spike {worst[1]:.3e}")
    assert ve[0] == 0.0
