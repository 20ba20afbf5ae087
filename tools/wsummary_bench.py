"""Device time of the weighted ensemble summary (odef_wsummary_field) beside the unweighted one: Lorenz-63 EK1(3),
N trajectories x n_steps steps, every step saved, filter + smoother, then both summaries of the filter (source 0) and smoothed
(source 1) records, best of `--repeat` from odef_kernel_time_ms(ctx, 7) and (ctx, 2) in the same process.  The weights are
synthetic log-likelihoods held in device memory.  With --baseline the same weighted summary the way a user of the library had to
take it before: odef_get of the two record fields plus a numpy reduction on the host (needs the records in host memory: use
--traj 4096).  Prints one JSON line.  Run it in a process of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import odefilters_jl_amd as pkg  # noqa: E402
from odefilters_jl_amd import host  # noqa: E402


def numpy_weighted_summary(mean, cov, rc, logw, d):
    tri = d * (d + 1) // 2
    il = np.tril_indices(d)
    ok = (rc == 0) & np.isfinite(logw)
    L = logw[ok].max()
    v = np.where(ok, np.exp(logw - L), 0.0)
    inc = ok[None, :] & np.all(np.isfinite(mean[:, :d, :]), axis=1)  # [n_t, N]
    vi = np.where(inc, v[None, :], 0.0)
    n = inc.sum(axis=1)
    Z = vi.sum(axis=1)
    m = (vi[:, None, :] * np.where(inc[:, None, :], mean[:, :d, :], 0.0)).sum(axis=2) / Z[:, None]
    w = (vi[:, None, :] * np.where(inc[:, None, :], cov[:, :tri, :], 0.0)).sum(axis=2) / Z[:, None]
    xc = np.where(inc[:, None, :], mean[:, :d, :] - m[:, :, None], 0.0)
    b = (vi[:, None, :] * xc[:, il[0], :] * xc[:, il[1], :]).sum(axis=2) / Z[:, None]
    return n, m, w, b, L + np.log(Z) - np.log(n), Z * Z / (vi * vi).sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # torch's HIP runtime first: brought up after the library's context it has been seen to find no GPU
    N, ns, d = a.traj, a.nsteps, 3
    tri = d * (d + 1) // 2
    problem = ([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx = pkg.Context("lorenz63", 3, host.EK1_ID, N, smooth=True)
    ctx.set_problem_perturbed(*problem)
    ctx.solve_fixed(np.arange(ns + 1) * 2.0**-9)
    ctx.smooth()
    logw = -100.0 - 20.0 * np.random.default_rng(0).standard_normal(N) ** 2
    unweighted_bytes = 8 * N * (ns + 1) * (2 * d + tri)
    out = {"traj": N, "n_t": ns + 1, "d": d, "algorithmic_bytes": unweighted_bytes + 2 * 8 * N * (ns + 1),
           "unweighted_algorithmic_bytes": unweighted_bytes}
    ctx.weighted_moments(0, logw)  # uploads and binds the weights once
    for source in (0, 1):
        best = {7: None, 2: None}
        for _ in range(a.repeat + 1):  # the first request is the warm-up
            ctx.set_problem_perturbed(*problem)  # drops both caches, keeps the records
            t0 = time.perf_counter()
            ctx.weighted_moments(source)
            wall = (time.perf_counter() - t0) * 1e3
            ctx.ensemble_moments(source)
            for which in best:
                ms = ctx.kernel_time_ms(which)[0]
                best[which] = ms if best[which] is None else min(best[which], ms)
        out[f"source{source}_ms"] = round(best[7], 4)
        out[f"source{source}_wall_ms"] = round(wall, 3)
        out[f"source{source}_unweighted_ms"] = round(best[2], 4)
        out[f"source{source}_ratio"] = round(best[7] / best[2], 3)
        out[f"source{source}_fraction_of_8TBps"] = round(out["algorithmic_bytes"] / (best[7] * 1e-3) / 8e12, 4)
    out["kernel"] = ctx.kernel_name(7)
    out["launches"] = ctx.kernel_time_ms(7)[1]
    if a.baseline:
        t0 = time.perf_counter()
        mean, cov, rc = ctx.get(host.F_MEAN), ctx.get(host.F_COV_TRIL), ctx.get(host.F_RETCODE)
        t1 = time.perf_counter()
        ref = numpy_weighted_summary(mean, cov, rc, logw, d)
        t2 = time.perf_counter()
        got = ctx.weighted_moments(0)
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_ms"] = round((t2 - t1) * 1e3, 1)
        out["baseline_max_abs_diff_mean"] = float(np.abs(ref[1] - got[1]).max())
        out["baseline_max_abs_diff_ess"] = float(np.abs(ref[5] - got[5]).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
