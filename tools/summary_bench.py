"""Device time of the ensemble summary (odef_summary_field): Lorenz-63 EK1(3), N trajectories x n_steps steps, every
step saved, filter + smoother, then the summary of the filter (source 0) and smoothed (source 1) records, best of `--repeat`
from odef_kernel_time_ms(ctx, 2).  With --baseline the same summary the way a user of the library had to take it before: odef_get
of the two record fields plus a two-pass numpy reduction on the host (needs the records in host memory: use --traj 4096).
Prints one JSON line.  Run it in a process of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odefilters_jl_amd as pkg  # noqa: E402
from odefilters_jl_amd import host  # noqa: E402


def numpy_summary(mean, cov, rc, d):
    tri = d * (d + 1) // 2
    il = np.tril_indices(d)
    inc = (rc == 0)[None, :] & np.all(np.isfinite(mean[:, :d, :]), axis=1)  # [n_t, N]
    n = inc.sum(axis=1)
    x = np.where(inc[:, None, :], mean[:, :d, :], 0.0)
    m = x.sum(axis=2) / n[:, None]
    w = np.where(inc[:, None, :], cov[:, :tri, :], 0.0).sum(axis=2) / n[:, None]
    xc = np.where(inc[:, None, :], mean[:, :d, :] - m[:, :, None], 0.0)
    b = (xc[:, il[0], :] * xc[:, il[1], :]).sum(axis=2) / n[:, None]
    return n, m, w, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    N, ns, d = a.traj, a.nsteps, 3
    tri = d * (d + 1) // 2
    ctx = pkg.Context("lorenz63", 3, host.EK1_ID, N, smooth=True)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx.solve_fixed(np.arange(ns + 1) * 2.0**-9)
    ctx.smooth()
    out = {"traj": N, "n_t": ns + 1, "d": d, "algorithmic_bytes": 8 * N * (ns + 1) * (2 * d + tri)}
    for source in (0, 1):
        best = None
        for _ in range(a.repeat + 1):  # the first request is the warm-up
            ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)  # drops the cache, keeps the records
            t0 = time.perf_counter()
            ctx.ensemble_moments(source)
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.kernel_time_ms(2)[0]
            best = ms if best is None else min(best, ms)
        out[f"source{source}_ms"] = round(best, 4)
        out[f"source{source}_wall_ms"] = round(wall, 3)
        out[f"source{source}_fraction_of_8TBps"] = round(out["algorithmic_bytes"] / (best * 1e-3) / 8e12, 4)
    out["kernel"] = ctx.kernel_name(2)
    if a.baseline:
        t0 = time.perf_counter()
        mean, cov, rc = ctx.get(host.F_MEAN), ctx.get(host.F_COV_TRIL), ctx.get(host.F_RETCODE)
        t1 = time.perf_counter()
        ref = numpy_summary(mean, cov, rc, d)
        t2 = time.perf_counter()
        got = ctx.ensemble_moments(0)
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_ms"] = round((t2 - t1) * 1e3, 1)
        out["baseline_max_abs_diff_mean"] = float(np.abs(ref[1] - got[1]).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
