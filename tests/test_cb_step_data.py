"""The premises of tests/test_gpu_cb_step_known_answer.py, pinned without a GPU
(tests/general_data.py): on every (N, m, j) and operator the GPU tests run,
a correct float64 step on the planted float columns with a summation tree of its own
(reversed 512-element partials) and one round-to-nearest conversion of w / h

  * keeps every Hessenberg entry below 1/8 of 64 eps ||w0|| ||V_i||, and
  * stores a column that meets |stored - v_ref| <= ulp32(v_ref) / 2 + 64 eps max |v_ref|
    element by element (the figures printed: how much of the 64 eps allowance it uses and
    how many elements differ from float32(v_ref));

and each seeded fault exceeds one of the two bounds.  The last three faults (a truncating
conversion, w / h divided in float, h rounded to float first) leave h untouched: only the
column criterion sees them.  The plans of k_mgs_wcb the resident cases name are pinned
against gk_cb_plan_query (pure host)."""
import numpy as np
import pytest

from tests.general_data import (CB_LAUNCH_SHAPES, MG_PARAMS, PARAMS, PREC_STEP_CASES, CB_RES_JS, CB_RES_M, CB_RES_PLANS, assert_asymmetric,
                                cb_column_excess, cb_planted, cb_step_ld, locate_cb, op_w0, planted_basis,
                                planted_basis_f32, step_bounds, ulp32)

FAULTS_H = ("dot_tail", "axpy1", "axpy2", "one_pass", "swap_halves")
FAULTS_COLUMN = ("truncate", "float_divide", "float_h")


def _dot_tree(a, b, skip_last=False):
    """Float64 dot with a summation tree of its own: 512-element partials, summed in reverse."""
    p = a * b
    if skip_last:
        p = p[:-1]
    s = 0.0
    for x in reversed([float(np.sum(p[k:k + 512])) for k in range(0, p.size, 512)]):
        s += x
    return s


def _swap_halves(v):
    """The two float2 halves of every whole 16-byte group exchanged: what a float4 pair load
    handed to the wrong slots reads."""
    out = v.copy()
    q = v.size // 4 * 4
    g = v[:q].reshape(-1, 4)
    out[:q] = g[:, [2, 3, 0, 1]].reshape(-1)
    return out


def _truncate32(x):
    f = x.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x)
    f[over] = np.nextafter(f[over], np.float32(0.0))
    return f


def _step_f64(V, w0, fault=None):
    """The FP32-basis step in float64 with _dot_tree: (h, the stored float column widened)."""
    j = V.shape[0]
    w = w0.copy()
    h = np.zeros(j + 1)
    hit = j // 2
    for p in range(1 if fault == "one_pass" else 2):
        for i in range(j):
            col = _swap_halves(V[i]) if fault == "swap_halves" and p == 0 and i == hit else V[i]
            d = _dot_tree(w, col, skip_last=(fault == "dot_tail" and p == 0 and i == hit))
            upd = w - d * col
            if fault == f"axpy{p + 1}" and i == hit:
                c = (w.size // 512) // 2 * 512
                upd[c:c + 512] = w[c:c + 512]
            w = upd
            h[i] += d
    h[j] = np.sqrt(_dot_tree(w, w))
    if fault == "truncate":
        f = _truncate32(w / h[j])
    elif fault == "float_divide":
        f = w.astype(np.float32) / np.float32(h[j])
    elif fault == "float_h":
        f = (w / np.float64(np.float32(h[j]))).astype(np.float32)
    else:
        f = (w / h[j]).astype(np.float32)
    assert f.dtype == np.float32
    return h, f.astype(np.float64)


def _ratios(h, stored, V, w0, ref):
    """(largest h deviation / bound, largest column excess over ulp32 / 2 in units of vb,
    elements that differ from float32(v_ref))."""
    hb, _ = step_bounds(V, w0, ref[1])
    exc, _ = cb_column_excess(stored, ref[1])
    n_off = int(np.count_nonzero(stored != ref[1].astype(np.float32).astype(np.float64)))
    return float(np.max(np.abs(h - ref[0]) / hb)), float(np.max(exc)), n_off


def _pin_cases():
    out = [(N, m, j, "left", "identity", 1) for N, m in CB_LAUNCH_SHAPES for j in (1, 2, m)]
    out += [(N, CB_RES_M, j, "left", "identity", 1) for N in sorted({p[0] for p in CB_RES_PLANS}) for j in CB_RES_JS]
    for _, side, prec, deg, _, N, m, params in PREC_STEP_CASES:
        assert params == (MG_PARAMS if prec == "mg" else PARAMS)  # the test below derives them from prec
        out += [(N, m, j, side, prec, deg) for j in (1, 2, m)]
    return sorted(set(out))


def test_planted_float_columns():
    N, m = 45, 8
    V32 = planted_basis_f32(N, m, seed=7000 + 7 * N + m)
    V = cb_planted(N, m)
    assert V32.dtype == np.float32 and V.dtype == np.float64 and np.array_equal(V, V32.astype(np.float64))
    V64 = planted_basis(N, m, seed=7000 + 7 * N + m)
    assert 0 < np.max(np.abs(V - V64)) <= 2.0 ** -24 * np.max(np.abs(V64))  # rounded once
    for k in range(m):
        assert_asymmetric(V[k], N)
    gram = V @ V.T - np.eye(m)
    assert 1e-7 < np.max(np.abs(gram)) < 1e-2


def test_ulp32():
    x = np.array([1.0, 1.5, 2.0 - 2.0 ** -30, 2.0, 0.75, -3.0, 0.0, 1e-46], dtype=np.longdouble)
    want = [2.0 ** -23, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]
    assert np.array_equal(ulp32(x), np.array(want))
    y = np.random.default_rng(3).standard_normal(1000)
    assert np.all(np.abs(y.astype(np.float32).astype(np.float64) - y) <= 0.5 * ulp32(y))


@pytest.mark.parametrize("N,m,j,side,prec,deg", _pin_cases())
def test_cb_step_bounds_pass_a_reordered_step(oracle, N, m, j, side, prec, deg):
    V = cb_planted(N, m)[:j]
    w0 = op_w0(oracle, V[j - 1], N, side, prec, deg, MG_PARAMS if prec == "mg" else PARAMS)
    ref = cb_step_ld(V, w0)
    assert abs(float(np.sqrt(np.dot(ref[1], ref[1]))) - 1.0) < 1e-14
    rh, rv, n_off = _ratios(*_step_f64(V, w0), V, w0, ref)
    print(f"N={N} m={m} j={j} {side} {prec}({deg}): reordered float64 step, h dev/bound {rh:.4f}, column "
          f"(dev - ulp32/2)/vb {rv:.4f}, {n_off} elements off float32(v_ref)")
    assert rh <= 1.0 / 8
    assert rv <= 1.0


@pytest.mark.parametrize("N,m,j", [(45, 8, 5), (130, 6, 6), (259, 8, 8), (309, 8, 5)])
def test_cb_step_bounds_fail_seeded_faults(oracle, N, m, j):
    V = cb_planted(N, m)[:j]
    w0 = op_w0(oracle, V[j - 1], N)
    ref = cb_step_ld(V, w0)
    good = _step_f64(V, w0)
    for fault in FAULTS_H + FAULTS_COLUMN:
        h, stored = _step_f64(V, w0, fault)
        fh, fv, n_off = _ratios(h, stored, V, w0, ref)
        print(f"N={N} j={j}: {fault}: h dev/bound {fh:.3e}, column excess/vb {fv:.3e}, {n_off} elements off "
              f"float32(v_ref)")
        if fault in FAULTS_COLUMN:  # h is the good step's, bit for bit: the column criterion alone
            assert np.array_equal(h, good[0])
            assert fv > 10.0, fault
        else:
            assert max(fh, fv) > 10.0, fault


@pytest.mark.parametrize("N,m", [(45, 12), (130, 10)])
def test_right_cbpr2_update_bound(oracle, N, m):
    """The bound of the right-preconditioned gk_update_x case, 64 eps |M^-1| sum_k |y_k V_k|
    (general_data.cbpr2_abs): the float64 evaluation x0 + cbpr2(V y) -- the oracle's cbpr2 on
    a sequentially summed V y -- stays below 1/8 of it against the long-double evaluation,
    with x0 = 0 and with a planted x0; x0 + V y (the sweep left out, or the left-side form
    launched) and M^-1 (V y) alone (x overwritten) exceed it."""
    from tests.general_data import EPS, MARGIN, cbpr2_abs, cbpr2_ld

    V = cb_planted(N, m)
    for n_out in (1, m):
        rng = np.random.default_rng(977 + n_out)
        y = rng.standard_normal(n_out)
        t_ld = (y.astype(np.longdouble)[:, None] * V[:n_out].astype(np.longdouble)).sum(axis=0)
        mag = cbpr2_abs(oracle, (np.abs(y)[:, None] * np.abs(V[:n_out])).sum(axis=0), N)
        z_ld = cbpr2_ld(oracle, t_ld, N)
        t = np.zeros(N * N)
        for k in range(n_out):
            t = t + V[k] * y[k]
        z = oracle.precond(oracle.PREC_CBPR2, t, N)
        for x0 in (np.zeros(N * N), rng.uniform(-1.0, 1.0, N * N) * mag):
            ref = x0.astype(np.longdouble) + z_ld
            ratio = lambda x: float(np.max(np.abs(x.astype(np.longdouble) - ref).astype(np.float64) / (MARGIN * EPS * mag)))  # noqa: E731
            good, no_sweep, overwritten = ratio(x0 + z), ratio(x0 + t), ratio(z)
            print(f"N={N} n_out={n_out} x0 {'planted' if np.any(x0) else 'zero'}: float64 dev/bound {good:.4f}; "
                  f"sweep left out {no_sweep:.3e}; x overwritten {overwritten:.3e}")
            assert good <= 1.0 / 8
            assert no_sweep > 10.0
            assert overwritten > 10.0 or not np.any(x0)


@pytest.mark.parametrize("N,wg,r2e,l2e,stream2,odd", CB_RES_PLANS)
def test_cb_resident_plans(N, wg, r2e, l2e, stream2, odd):
    """The plans the resident GPU cases assert, from gk_cb_plan_query on 256 CUs; which
    workgroups hold pairs, a single chunk or nothing follows from them (locate_cb)."""
    import gmres_amd as ga

    n = N * N
    p = ga.cb_plan_query(n, cus=256, share=256 // wg, m=CB_RES_M)
    print(f"N={N} on {wg} workgroups: {p}")
    assert p["on"] and p["G"] == wg
    assert (p["r2e"], p["l2e"], p["nstream2"], bool(n & 1)) == (r2e, l2e, stream2, odd), p
    plan = {"variant": "compressed-basis", "wt": 256, "G": wg, "r2e": r2e, "l2e": l2e, "r2": p["rw"], "l2": p["lw"],
            "nres2": p["nres2"]}
    nch = p["nres2"] // 256
    held = [max(0, min(r2e, nch - g * r2e)) for g in range(wg)]
    print(f"  register chunks per workgroup {held}")
    if (N, wg) == (130, 2):
        assert held == [17, 16]
    if (N, wg) == (130, 4):
        assert held == [9, 9, 9, 6]
    if (N, wg) == (130, 16):
        assert held[:11] == [3] * 11 and held[11:] == [0] * 5
    # every element has one home, and the two double2 a lane owns in a pair are neighbours
    where = [locate_cb(e, plan, n) for e in (0, 1, 2, 3, 511, 512, 2 * p["nres2"] - 1, n - 1)]
    assert "half 0" in where[0] or "unpaired" in where[0]
    assert where[0] == where[1] and (where[2] != where[0])
    if p["nstream2"]:
        assert "streamed" in locate_cb(2 * p["nres2"], plan, n)
    if odd:
        assert "tail" in where[-1]
    if held[0] >= 2:
        assert "half 0" in where[0] and "half 1" in where[2] and "lane 0," in where[2] + ","
        assert "lane 1," in locate_cb(4, plan, n) + "," and "lane 255," in locate_cb(1023, plan, n) + ","
