#!/usr/bin/env python3
"""The CGS2 Arnoldi step (gk_set_orthogonalization GK_ORTH_CGS2) against the MGS-R step, same
process, one context per leg: GMRES(m), identity preconditioner, one GPU.

Four legs, interleaved sample by sample:

  resident   the default MGS-R step (one resident launch per Arnoldi step)
  launch     the launch-path MGS-R step (GK_TUNE_RES 0, hipGraph replays): 2j + 1 launches
  cgs2_kb8   CGS2 with batches of 8 columns in the dots kernel (GK_CGS_KB=8 at gk_create)
  cgs2_kb16  ... of 16

Per leg one untimed solve, then --samples samples of --cycles timed restart cycles each (the
region bench.py times: whole cycles through the Fortran host driver).  One JSON line per
sample with it_s, the Arnoldi steps per second.  Then one cycle per leg with graphs off and
the profiler on: the ms per kernel class of gk_profile_read, and for the CGS2 legs the
fraction of HBM bandwidth their dots + AXPY launches reach under the byte model

  dots  8 n (j + ceil(j / KB))     AXPY  8 n (j + 2)     per sweep, two sweeps per step.

The closing line holds, per leg, the slowest / median / fastest it_s, the ratios of the medians
and `cgs2_beats_launch`: the slowest CGS2 sample is faster than the fastest launch-path sample.

  python tools/cgs2_bench.py [--grid 4096] [--m 95] [--samples 3] [--cycles 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
LEGS = ("resident", "launch", "cgs2_kb8", "cgs2_kb16")


def cgs2_proj_bytes(j: int, n: int, kb: int) -> float:
    """Bytes the four projection-class launches of CGS2 step j move under the byte model."""
    return 2 * (8.0 * n * (j + -(-j // kb)) + 8.0 * n * (j + 2))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--m", type=int, default=95)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=2)
    a = ap.parse_args()
    import gmres_amd as ga
    from gmres_amd import _native as nat

    m, n = a.m, a.grid * a.grid
    its = {leg: [] for leg in LEGS}
    prof = {}
    ctxs = {}
    try:
        # one context per leg, configured once: a tuning call drops the captured step graphs, and
        # re-capturing them inside a timed sample would charge the launch-path legs for it
        for leg in LEGS:
            if leg.startswith("cgs2"):
                os.environ["GK_CGS_KB"] = leg[7:]  # read by gk_create
            c = ctxs[leg] = ga.Context(a.grid, m)
            os.environ.pop("GK_CGS_KB", None)
            c.set_precond("identity")
            c.set_rhs_ones()
            c.set_orth("cgs2" if leg.startswith("cgs2") else "mgsr")
            if leg == "launch":
                c.tune(nat.GK_TUNE_RES, 0)

        def solve(c, cycles):
            r = ga.gmres_mgsr(c, 1e-15, max_cycles=cycles, want_verr=False, want_hist=True, want_x=False)
            c.sync()
            return [int(np.count_nonzero(row)) for row in r.hist_ferr]  # Arnoldi steps of every cycle

        for leg in LEGS:
            solve(ctxs[leg], 1)  # untimed: captures the step graphs
        for s in range(a.samples):
            for leg in LEGS:
                c = ctxs[leg]
                variant = c.res_info()["variant"]
                t0 = time.perf_counter()
                steps = solve(c, a.cycles)
                dt = time.perf_counter() - t0
                it_s = sum(steps) / dt
                its[leg].append(it_s)
                print(json.dumps({"grid": a.grid, "m": m, "leg": leg, "sample": s, "variant": variant,
                                  "cycles": len(steps), "steps": sum(steps), "seconds": round(dt, 4),
                                  "it_s": round(it_s, 2)}), flush=True)
        for leg in LEGS:  # one profiled cycle, launch by launch
            c = ctxs[leg]
            c.tune(nat.GK_TUNE_GRAPH, 0)
            c.profile(True)
            c.profile_reset()
            steps = solve(c, 1)
            p = {k: (round(ms, 3), cnt) for k, (ms, cnt) in c.profile_read().items() if cnt > 0}
            c.profile(False)
            prof[leg] = {"steps": sum(steps), "ms": p}
            if leg.startswith("cgs2"):
                by = sum(cgs2_proj_bytes(j, n, int(leg[7:])) for k in steps for j in range(1, k + 1))
                prof[leg]["proj_bytes"] = round(by)
                prof[leg]["proj_hbm_frac"] = round(by / (p["proj"][0] * 1e-3) / HBM_BYTES_PER_S, 4)
            print(json.dumps({"grid": a.grid, "m": m, "leg": leg, "profile": prof[leg]}), flush=True)
    finally:
        for c in ctxs.values():
            c.close()
    stat = {leg: {"min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2)}
            for leg, v in its.items()}
    med = {leg: statistics.median(v) for leg, v in its.items()}
    best = max(("cgs2_kb8", "cgs2_kb16"), key=lambda leg: med[leg])
    print(json.dumps({"grid": a.grid, "m": m, "samples": a.samples, "cycles": a.cycles, "it_s": stat,
                      "best_cgs2": best,
                      "cgs2_over_launch": round(med[best] / med["launch"], 4),
                      "cgs2_over_resident": round(med[best] / med["resident"], 4),
                      "kb16_over_kb8": round(med["cgs2_kb16"] / med["cgs2_kb8"], 4),
                      "cgs2_beats_launch": bool(min(min(its["cgs2_kb8"]), min(its["cgs2_kb16"])) > max(its["launch"]))}),
          flush=True)


if __name__ == "__main__":
    main()
