"""Device time of the event location pass (odef_event_field): Lorenz-63 EK1(3), N trajectories x 1 024 steps, every
step saved (1 025 saves), component 0, level 0, both directions, K = 4, both sources; best of `--repeat` after a warm-up from
odef_kernel_time_ms(ctx, 5) (scan + refinement; the scan's share of the 8 TB/s peak is quoted against the whole pass, so it is a lower
bound).  With --baseline, in the same process, a LOWER bound of the only route there was before: odef_get of MEAN (smoothed), the
numpy sign scan, and one odef_dense_output launch per Newton iterate and slot at ONE shared time (that route cannot evaluate every
trajectory at its own time; it needs the records in host memory: use --traj 4096).  Prints one JSON line.  Run it in a process of its
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
import odefilters_jl_amd as pkg  # noqa: E402
from odefilters_jl_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()  # torch's HIP runtime first: brought up after the library's context it has been seen to find no GPU
    N, ns, q, K = a.traj, a.nsteps, 3, a.slots
    grid = np.arange(ns + 1) * 2.0**-9
    ctx = pkg.Context("lorenz63", q, host.EK1_ID, N, smooth=True)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx.solve_fixed(grid)
    ctx.smooth()
    spec, level = host._to_device((np.array([0, 0, K], np.int64), np.zeros(1)), ctx.cfg.device)
    out = {"traj": N, "n_save": ns + 1, "K": K, "scan_bytes": 8 * N * (ns + 1)}
    for source, key in ((0, "filter"), (1, "smoothed")):
        best = None
        for _ in range(a.repeat + 1):  # the first request is the warm-up
            ctx.bind_event(spec.data_ptr(), level.data_ptr(), False)  # drops the cache, keeps everything else
            t0 = time.perf_counter()
            ev = ctx.events(source)
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.kernel_time_ms(host.K_EVENTS)[0]
            best = ms if best is None else min(best, ms)
        located = ev.save >= 0
        out[f"{key}_ms"] = round(best, 4)
        out[f"{key}_wall_ms"] = round(wall, 3)
        out[f"{key}_scan_fraction_of_8TBps_at_least"] = round(out["scan_bytes"] / (best * 1e-3) / 8e12, 4)
        out[f"{key}_events_located"] = int(located.sum())
        out[f"{key}_count_max"] = int(ev.count.max())
        out[f"{key}_neval_max_median"] = [int(ev.neval[located].max()), float(np.median(ev.neval[located]))] if located.any() else None
    out["kernel"] = ctx.kernel_name(host.K_EVENTS)
    if a.baseline:
        t0 = time.perf_counter()
        mean = ctx.get(host.F_SMOOTH_MEAN)                       # [n_save, D, N]
        t1 = time.perf_counter()
        g = mean[:, 0, :]
        cross = ((g[:-1] < 0) & (g[1:] >= 0)) | ((g[:-1] > 0) & (g[1:] <= 0))
        first = np.argmax(cross, axis=0)
        t2 = time.perf_counter()
        launches = 5 * K                                          # the median iterate count of the device pass, per slot
        for j in range(launches):
            ctx.dense_output(np.array([grid[int(first[0])] + 2.0**-10 * (1 + j / launches)]), True)
        t3 = time.perf_counter()
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_scan_ms"] = round((t2 - t1) * 1e3, 1)
        out["baseline_dense_launches"] = launches
        out["baseline_dense_ms"] = round((t3 - t2) * 1e3, 1)
        out["baseline_over_events_at_least"] = round((t3 - t0) * 1e3 / out["smoothed_ms"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
