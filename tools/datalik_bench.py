"""Device time of the data log-likelihood pass (odef_data_field): Lorenz-63 EK1(3), N trajectories x 1 024 steps,
every step saved (1 025 saves), 129 observations (every 8th save) of all three components, best of `--repeat` after a warm-up from
odef_kernel_time_ms(ctx, 4).  Beside it, in the same process: the smoother's kernel time on the same records (which = 1) -- the
launcher's choice for this N and the lane smoother forced --, and with --baseline the only route there was before: odef_get of MEAN,
COV_TRIL and DIFFUSION plus the numpy float64 evaluation of tests/_datalik_reference.py on the host (needs the records in host
memory: use --traj 4096).  Prints one JSON line.  Run it in a process of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import odefilters_jl_amd as pkg  # noqa: E402
from odefilters_jl_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime first: brought up after the library's context it has been seen to find no GPU
    N, ns, d, q = a.traj, a.nsteps, 3, 3
    D = d * (q + 1)
    tri = D * (D + 1) // 2
    grid = np.arange(ns + 1) * 2.0**-9
    ctx = pkg.Context("lorenz63", q, host.EK1_ID, N, smooth=True)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx.solve_fixed(grid)
    saves = np.arange(0, ns + 1, a.every, dtype=np.int64)
    comps = np.arange(d, dtype=np.int64)
    # the data: the unperturbed trajectory's own filter means at the observed saves plus N(0, 1e-4) noise, fetched row by row
    rng = np.random.default_rng(7)
    tight = pkg.Context("lorenz63", q, host.EK1_ID, 1)
    tight.set_problem(np.array([[1.0, 0.0, 0.0]]), np.array([10.0, 28.0, 8.0 / 3.0]), 0.0)
    tight.solve_fixed(grid)
    y = tight.get(host.F_MEAN)[saves, :d, 0] + 1e-2 * rng.standard_normal((len(saves), d))
    tight.close()
    noise = np.full(d, 1e-4)
    bufs = host._to_device((saves, comps, y, noise), ctx.cfg.device)
    ctx.bind_observations(*[b.data_ptr() for b in bufs], len(saves), d, False)
    out = {"traj": N, "n_save": ns + 1, "observations": int(len(saves)), "o": d,
           "algorithmic_bytes": 8 * N * (ns + 1) * (D + tri + 1)}
    best = None
    for _ in range(a.repeat + 1):  # the first request is the warm-up
        ctx.bind_device(host.L_OBS_NOISE, bufs[3].data_ptr(), 8 * d)  # drops the cache, keeps everything else
        t0 = time.perf_counter()
        ll, mq = ctx.data_loglik()
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctx.kernel_time_ms(host.K_DATA_LOGLIK)[0]
        best = ms if best is None else min(best, ms)
    out["datalik_ms"] = round(best, 4)
    out["datalik_wall_ms"] = round(wall, 3)
    out["fraction_of_8TBps"] = round(out["algorithmic_bytes"] / (best * 1e-3) / 8e12, 4)
    out["kernel"] = ctx.kernel_name(host.K_DATA_LOGLIK)
    out["median_mahalanobis"] = float(np.median(mq))
    out["argmax"] = int(np.argmax(ll))
    # the smoother on the same records: the launcher's choice, then the lane smoother forced
    for key, env in (("smoother", {}), ("lane_smoother", {"ODEF_SMOOTH_ROWS_MAX_N": "0", "ODEF_SMOOTH_LANE_MIN_N": "0"})):
        os.environ.update(env)
        sm = None
        for _ in range(a.repeat + 1):
            ctx.smooth()
            t = ctx.kernel_time_ms(1)[0]
            sm = t if sm is None else min(sm, t)
        out[f"{key}_ms"] = round(sm, 4)
        out[f"{key}_kernel"] = ctx.kernel_name(1)
        for k in env:
            del os.environ[k]
    out["datalik_over_lane_smoother"] = round(best / out["lane_smoother_ms"], 3)
    if a.baseline:
        import _datalik_reference as dr

        t0 = time.perf_counter()
        mean, cov, diff = ctx.get(host.F_MEAN), ctx.get(host.F_COV_TRIL), ctx.get(host.F_DIFFUSION)
        t1 = time.perf_counter()
        want = dr.evaluate(mean, cov, diff, grid, d, q, saves, comps, y, noise, dtype=np.float64)
        t2 = time.perf_counter()
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_ms"] = round((t2 - t1) * 1e3, 1)
        out["baseline_over_datalik"] = round((t2 - t0) * 1e3 / best, 1)
        out["baseline_max_rel_diff_loglik"] = float(np.max(np.abs(want["loglik"] - ll) / np.abs(want["loglik"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
