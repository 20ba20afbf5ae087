"""Device time of the data log-likelihood at arbitrary observation times (ODEF_L_OBS_TIME) beside the save path
(3.15) on the same inputs: Lorenz-63 EK1(3), N trajectories x 1 024 steps, every step saved (1 025 saves), 129 observation times
of all three components, best of `--repeat` after a warm-up from odef_kernel_time_ms(ctx, 4).
  save_path_ms       ODEF_L_OBS_SAVE: every 8th save
  time_on_grid_ms    ODEF_L_OBS_TIME: the times of those saves (the largest difference to the save path is printed)
  time_off_grid_ms   ODEF_L_OBS_TIME: those times moved 0.37 steps into their step (the last one 0.63 steps back)
With --adaptive: the same problem solved adaptively (capacity 1 025 records) and the time path on the off-grid times, beside the
only route there was before for an adaptive ensemble: odef_get of MEAN, COV_TRIL, DIFFUSION, T and NSAVED plus the numpy float64
evaluation of tests/_datalik_times_reference.py -- run on the first --baseline-lanes trajectories and scaled to N (every
trajectory has its own grid and is a sweep of its own there; use --traj 4096).  Prints one JSON line.  Run it in a process of its
own."""
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


def best_ms(ctx, bufs, d, repeat):
    best = None
    for _ in range(repeat + 1):  # the first request is the warm-up
        ctx.bind_device(host.L_OBS_NOISE, bufs[3].data_ptr(), 8 * d)  # drops the cache, keeps everything else
        ll, mq = ctx.data_loglik()
        ms = ctx.kernel_time_ms(host.K_DATA_LOGLIK)[0]
        best = ms if best is None else min(best, ms)
    return best, ll, mq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--baseline-lanes", type=int, default=16)
    a = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime is initialised before the library's context, as in tools/datalik_bench.py
    N, ns, d, q = a.traj, a.nsteps, 3, 3
    dt = 2.0**-9
    grid = np.arange(ns + 1) * dt
    u0, p = [1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0]
    ctx = pkg.Context("lorenz63", q, host.EK1_ID, N)
    ctx.set_problem_perturbed(u0, p, 0.0, 1e-3)
    ctx.solve_fixed(grid)
    saves = np.arange(0, ns + 1, a.every, dtype=np.int64)
    comps = np.arange(d, dtype=np.int64)
    rng = np.random.default_rng(7)
    tight = pkg.Context("lorenz63", q, host.EK1_ID, 1)
    tight.set_problem(np.array([u0]), np.array(p), 0.0)
    tight.solve_fixed(grid)
    y = tight.get(host.F_MEAN)[saves, :d, 0] + 1e-2 * rng.standard_normal((len(saves), d))
    tight.close()
    noise = np.full(d, 1e-4)
    off = grid[saves] + 0.37 * dt
    off[-1] = grid[saves[-1]] - 0.63 * dt
    out = {"traj": N, "n_save": ns + 1, "observations": int(len(saves)), "o": d}
    bufs = host._to_device((saves, comps, y, noise), ctx.cfg.device)
    ctx.bind_observations(*[b.data_ptr() for b in bufs], len(saves), d, False)
    out["save_path_ms"], ll_s, _ = best_ms(ctx, bufs, d, a.repeat)
    out["save_path_kernel"] = ctx.kernel_name(host.K_DATA_LOGLIK)
    for key, times in (("time_on_grid", grid[saves]), ("time_off_grid", off)):
        tb = host._to_device((times, comps, y, noise), ctx.cfg.device)
        ctx.bind_observation_times(*[b.data_ptr() for b in tb], len(times), d, False)
        out[key + "_ms"], ll, _ = best_ms(ctx, tb, d, a.repeat)
        out[key + "_kernel"] = ctx.kernel_name(host.K_DATA_LOGLIK)
        out[key + "_finite"] = int(np.isfinite(ll).sum())
        if key == "time_on_grid":
            out["on_grid_max_rel_diff_to_save_path"] = float(np.max(np.abs(ll - ll_s) / np.abs(ll_s)))
    if a.adaptive:
        import _datalik_times_reference as tr

        ctx.solve_adaptive(float(grid[-1]), dt0=dt, max_steps=ns)
        ns_i = ctx.get(host.F_NSAVED)
        out["adaptive_nsaved_min_max"] = [int(ns_i.min()), int(ns_i.max())]
        tb = host._to_device((off, comps, y, noise), ctx.cfg.device)
        ctx.bind_observation_times(*[b.data_ptr() for b in tb], len(off), d, False)
        out["adaptive_time_off_grid_ms"], ll, _ = best_ms(ctx, tb, d, a.repeat)
        out["adaptive_finite"] = int(np.isfinite(ll).sum())
        t0 = time.perf_counter()
        mean, cov, diff = ctx.get(host.F_MEAN), ctx.get(host.F_COV_TRIL), ctx.get(host.F_DIFFUSION)
        T = ctx.get(host.F_T)
        t1 = time.perf_counter()
        L = min(a.baseline_lanes, N)
        want = tr.evaluate(mean[:, :, :L], cov[:, :, :L], diff[:, :L], T[:, :L], d, q, off, list(comps), y, noise, ns_i[:L], dtype=np.float64)
        t2 = time.perf_counter()
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_lanes"] = L
        out["baseline_numpy_ms_measured_on_those_lanes"] = round((t2 - t1) * 1e3, 1)
        out["baseline_numpy_ms_scaled_to_all_lanes_not_measured"] = round((t2 - t1) * 1e3 * N / L, 1)
        fin = np.isfinite(ll[:L])
        out["baseline_max_rel_diff_loglik"] = float(np.max(np.abs(want["loglik"][fin] - ll[:L][fin]) / np.abs(want["loglik"][fin])))
    for k, v in out.items():
        if isinstance(v, float):
            out[k] = round(v, 4) if abs(v) >= 1e-3 else v
    print(json.dumps(out))


if __name__ == "__main__":
    main()
