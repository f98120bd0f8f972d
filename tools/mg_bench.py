#!/usr/bin/env python3
"""The multigrid preconditioner (GK_PREC_MG, its defaults: degree 2 on (8, 1)) against
Chebyshev(8) and cbpr2 on (8.2, 0.2), same process, one context per leg, one GPU:
wall time to a relative residual of 1e-8 from x0 = 0, b = A 1.

Legs, interleaved sample by sample:

  mg        the V-cycle with the fused residual-restriction (GK_TUNE_MG_FUSED 1, the default)
  mg_unf    ... with OP_RESID into a work vector and the plain restriction (GK_TUNE_MG_FUSED 0)
  cheb8     Chebyshev(8)
  cbpr2     the reference's two-term Chebyshev

and two solvers, one phase each: right-preconditioned MGS-R GMRES(m) through the Fortran
host driver (stops on |g| / ||b|| < tol, the true relative residual on the right), then PCG
by the fused short-recurrence driver (stops on ||r|| < tol ||b||).  A phase configures every
context, runs one untimed solve per leg (code objects, captured graphs), then --samples timed
solves of the multigrid legs and --baseline-samples of the others, capped at --max-cycles
restart cycles / --max-iter iterations (a capped solve is reported with converged false
and the residual it reached).  After the GMRES phase one more solve per multigrid leg runs
with the profiler on: the us per V-cycle is GK_KID_PREC's time over its count.

One JSON line per sample, per profile and a closing summary per solver (medians, the
ratios of the medians); the lines are also written to --out (default
profiles/mg/mg_bench_<grid>.jsonl; --append adds a run, e.g. a second m, to it).

  python tools/mg_bench.py [--grid 4096] [--m 95] [--samples 3] [--baseline-samples 1]
  python tools/mg_bench.py --grid 4096 --m 30 --max-cycles 60 --append

--shift SIGMA runs every leg on A + SIGMA I (gk_set_shift; b = (A + SIGMA I) 1, every interval
moved by SIGMA: the multigrid smoother's (8 + SIGMA, 1 + SIGMA), the others' (8.2 + SIGMA,
0.2 + SIGMA)); its records carry "shift".
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL = 1e-8
LEGS = ("mg", "mg_unf", "cheb8", "cbpr2")
MG_LEGS = ("mg", "mg_unf")


def vcycle_bytes(n: int, fused: bool) -> float:
    """The byte model of one V-cycle on n fine unknowns: per fine unknown of
    a level, each smoothing as one temporal-blocked pass 16, the residual-restriction 18 (34
    unfused), the prolongation 18, the post-smoothing residual 24, the closing add 24 -- 116
    (132); times 4/3 for the coarser levels."""
    return (4.0 / 3.0) * n * (16 + (18 if fused else 34) + 18 + 24 + 16 + 24)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--m", type=int, default=95)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--baseline-samples", type=int, default=1)
    ap.add_argument("--max-cycles", type=int, default=20)
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--shift", type=float, default=0.0, help="the operator is A + SHIFT I (default 0)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of rewriting it")
    a = ap.parse_args()
    import gmres_amd as ga
    from gmres_amd import _native as nat

    out_path = a.out or os.path.join(ROOT, "profiles", "mg", f"mg_bench_{a.grid}.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    out = open(out_path, "a" if a.append else "w")

    def emit(rec: dict) -> None:
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    m, n = a.m, a.grid * a.grid
    base = {"grid": a.grid, "m": m, "tol": TOL}
    sg = a.shift
    if sg != 0.0:
        base["shift"] = sg
    ctxs = {}

    def configure(c, leg, side):
        if leg in MG_LEGS:
            c.tune(nat.GK_TUNE_MG_FUSED, 1 if leg == "mg" else 0)
            c.set_precond("mg", (8.0 + sg, 1.0 + sg) if sg != 0.0 else None, side=side)
        elif leg == "cheb8":
            c.set_precond("cheb", (8.2 + sg, 0.2 + sg), 8, side=side)
        else:
            c.set_precond("cbpr2", (8.2 + sg, 0.2 + sg), side=side)

    def solve_gmres(c, cycles):
        t0 = time.perf_counter()
        r = ga.gmres_mgsr(c, TOL, max_cycles=cycles, want_verr=False, want_x=False)
        c.sync()
        dt = time.perf_counter() - t0
        return dt, r.iterations, r.n_cycles

    def solve_pcg(c, iters):
        t0 = time.perf_counter()
        _, it, res, _ = ga.pcg(c, tol=TOL * c.beta, max_iter=iters)
        c.sync()
        return time.perf_counter() - t0, it, 0

    try:
        for leg in LEGS:
            c = ctxs[leg] = ga.Context(a.grid, m)
            if sg != 0.0:
                c.set_shift(sg)
            c.set_rhs_ones()
            c.beta = c.rhs_norm()
        for solver, side, solve, cap, warm in (("mgsr_right", "right", solve_gmres, a.max_cycles, 1),
                                               ("pcg", "left", solve_pcg, a.max_iter, 40)):
            times = {leg: [] for leg in LEGS}
            iters = {}
            for leg in LEGS:
                configure(ctxs[leg], leg, side)
                solve(ctxs[leg], warm)  # untimed
            for s in range(max(a.samples, a.baseline_samples)):
                for leg in LEGS:
                    if s >= (a.samples if leg in MG_LEGS else a.baseline_samples):
                        continue
                    c = ctxs[leg]
                    dt, it, cyc = solve(c, cap)
                    res = c.true_residual()
                    times[leg].append(dt)
                    iters[leg] = it
                    emit({**base, "solver": solver, "leg": leg, "sample": s, "iterations": it, "cycles": cyc,
                          "seconds": round(dt, 5), "true_residual": res, "converged": bool(res < TOL)})
            if solver == "mgsr_right":  # a profiled solve of their own: us per V-cycle
                for leg in MG_LEGS:
                    c = ctxs[leg]
                    c.profile(True)
                    c.profile_reset()
                    solve(c, cap)
                    ms, cnt = c.profile_read()["prec"]
                    c.profile(False)
                    us = ms / cnt * 1e3
                    by = vcycle_bytes(n, leg == "mg")
                    emit({**base, "solver": solver, "leg": leg, "profile": {"vcycles": cnt, "us_per_vcycle": round(us, 2),
                                                                           "model_bytes": round(by),
                                                                           "model_tb_s": round(by / (us * 1e-6) / 1e12, 3)},
                          "levels": c.mg_info()["sides"]})
            med = {leg: statistics.median(v) for leg, v in times.items() if v}
            emit({**base, "solver": solver, "summary": {
                "seconds": {leg: {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
                                  "max": round(max(v), 5)} for leg, v in times.items() if v},
                "iterations": iters,
                "cheb8_over_mg": round(med["cheb8"] / med["mg"], 3) if "cheb8" in med else None,
                "cbpr2_over_mg": round(med["cbpr2"] / med["mg"], 3) if "cbpr2" in med else None,
                "mg_unf_over_mg": round(med["mg_unf"] / med["mg"], 4)}})
    finally:
        for c in ctxs.values():
            c.close()
        out.close()


if __name__ == "__main__":
    main()
