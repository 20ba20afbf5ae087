"""Device time of the ensemble quantiles (odef_quantile_field): Lorenz-63 EK1(3), N trajectories x n_steps steps,
every step saved, filter + smoother, then the quantiles (0.05, 0.5, 0.95) of the filter (source 0) and smoothed (source 1) records,
best of `--repeat` from odef_kernel_time_ms(ctx, 6).  --final: final-save mode (one record, no smoother).  With --baseline the same quantiles the way a
user of the library had to take them before: odef_get of the mean records plus np.quantile on the host, wall time against the wall
time of sol.quantiles' path (needs the records in host memory: use --traj 4096).  Prints one JSON line.  Run it in a process of
its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.05, 0.5, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--final", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first: brought up after the library's context it has been seen to find no GPU
    import odefilters_jl_amd as pkg
    from odefilters_jl_amd import host

    N, ns, d = a.traj, a.nsteps, 3
    ctx = pkg.Context("lorenz63", 3, host.EK1_ID, N, smooth=not a.final, save_everystep=not a.final)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx.solve_fixed(np.arange(ns + 1) * 2.0**-9)
    if not a.final:
        ctx.smooth()
    n_t = ctx.n_save
    slab = min(1024 // d, n_t)  # the pass works the times in slabs of 1024 / d (include/odefilter.h)
    n_slab = -(-n_t // slab)
    out = {"traj": N, "n_t": n_t, "d": d, "P": len(PROBS), "slab_times": slab, "slabs": n_slab,
           "filter_ms": round(ctx.kernel_time_ms(0)[0], 3)}
    for source in (0,) if a.final else (0, 1):
        best = None
        for _ in range(a.repeat + 1):  # the first request is the warm-up
            ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)  # drops the cache, keeps the records
            t0 = time.perf_counter()
            ctx.ensemble_quantiles(source, PROBS)
            wall = (time.perf_counter() - t0) * 1e3
            ms, nl = ctx.kernel_time_ms(6)
            best = ms if best is None else min(best, ms)
        passes = (nl - 4 * n_slab) / 2 / n_slab  # launches: 4 per slab and 2 per digit pass
        nbytes = 8 * N * n_t * d * (1 + passes) + n_t * N / 8 * (1 + passes * d)
        out[f"source{source}_ms"] = round(best, 4)
        out[f"source{source}_wall_ms"] = round(wall, 3)
        out[f"source{source}_launches"] = nl
        out[f"source{source}_passes_per_slab"] = round(passes, 2)
        out[f"source{source}_algorithmic_bytes"] = int(nbytes)
        out[f"source{source}_fraction_of_8TBps"] = round(nbytes / (best * 1e-3) / 8e12, 4)
    out["kernel"] = ctx.kernel_name(6)
    if not a.final:
        ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
        ctx.ensemble_moments(0)
        out["summary_ms"] = round(ctx.kernel_time_ms(2)[0], 4)
    if a.baseline:
        t0 = time.perf_counter()
        mean = ctx.get(host.F_MEAN)
        t1 = time.perf_counter()
        ref = np.quantile(mean[:, :d, :], PROBS, axis=-1).transpose(1, 0, 2)  # [n_t, P, d]
        t2 = time.perf_counter()
        ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
        got = ctx.ensemble_quantiles(0, PROBS)[1]
        t3 = time.perf_counter()
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_ms"] = round((t2 - t1) * 1e3, 1)
        out["device_wall_ms"] = round((t3 - t2) * 1e3, 2)
        out["baseline_max_rel_diff"] = float(np.max(np.abs(ref - got) / np.abs(ref)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
