#!/usr/bin/env python3
"""FP64 basis against the FP32-compressed basis (gk_set_basis_precision), same process,
same context: MGS-R GMRES(m), identity preconditioner, one GPU.

The two solves alternate.  Per precision one untimed cycle, then --samples samples of
--cycles timed cycles each (clock split off), each followed by one cycle with the
in-kernel clock split on (gk_profile_res_split) for the pass / wait figures.  One JSON
line per sample:

  it_s        Arnoldi steps per second of the timed cycles
  pass_us, wait_us   per projection, mean over workgroups
  step_bytes  mean bytes per Arnoldi step under the byte model of the variant:
                f64  (16 * 2j + 8 + 8) n   two FP64 columns per projection, w in, the column out
                f32  ( 8 * 2j + 8 + 4 + 8) n   float columns, w in, the float column out, vjw out
  hbm_frac    step_bytes * it_s over 8 TB/s

and a closing line with the f32 / f64 ratio of the medians.

  python tools/cb_bench.py [--grid 4096] [--m 95] [--samples 3] [--cycles 5]
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


def model_bytes(basis: str, j: int, n: int) -> float:
    return ((16 * 2 * j + 8 + 8) if basis == "f64" else (8 * 2 * j + 8 + 4 + 8)) * n


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--m", type=int, default=95)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=5)
    a = ap.parse_args()
    import gmres_amd as ga

    m, n = a.m, a.grid * a.grid
    its = {"f64": [], "f32": []}
    with ga.Context(a.grid, m) as c:
        c.set_precond("identity")
        c.set_rhs_ones()

        def solve(cycles):
            r = ga.gmres_mgsr(c, 1e-15, max_cycles=cycles, want_verr=False, want_hist=True, want_x=False)
            c.sync()
            return [int(np.count_nonzero(row)) for row in r.hist_ferr]  # Arnoldi steps of every cycle

        for basis in ("f64", "f32"):
            c.set_basis(basis)
            solve(1)
        for s in range(a.samples):
            for basis in ("f64", "f32"):
                c.set_basis(basis)
                info = c.res_info()
                t0 = time.perf_counter()
                steps = solve(a.cycles)
                dt = time.perf_counter() - t0
                c.res_split(1)
                split_steps = solve(1)
                r = c.res_split(-1, 0)
                c.res_split(0)
                nproj = sum(j * (j + 1) for j in split_steps)  # 2j projections per step j
                it_s = sum(steps) / dt
                step_bytes = sum(model_bytes(basis, j, n) for k in steps for j in range(1, k + 1)) / sum(steps)
                its[basis].append(it_s)
                print(json.dumps({"grid": a.grid, "m": m, "basis": basis, "sample": s, "variant": info["variant"],
                                  "r2e": info["r2e"], "l2e": info["l2e"], "cycles": len(steps), "steps": sum(steps),
                                  "seconds": round(dt, 4), "it_s": round(it_s, 2),
                                  "pass_us": round(r["pass_ms"] * 1e3 / nproj, 3),
                                  "wait_us": round(r["wait_ms"] * 1e3 / nproj, 3),
                                  "step_bytes": round(step_bytes), "hbm_frac": round(step_bytes * it_s / HBM_BYTES_PER_S, 4)}),
                      flush=True)
    med = {b: statistics.median(v) for b, v in its.items()}
    print(json.dumps({"grid": a.grid, "m": m, "median_it_s": {b: round(v, 2) for b, v in med.items()},
                      "f32_over_f64": round(med["f32"] / med["f64"], 4)}), flush=True)


if __name__ == "__main__":
    main()
