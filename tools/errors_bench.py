"""Device time of the per-trajectory solution errors (odef_errors_field): Lorenz-63 EK1(3), N trajectories x n_steps
steps, every step saved, filter + smoother, a reference buffer [n_save][3][N] bound as the truth, then the errors of the filter
(source 0) and smoothed (source 1) records, best of `--repeat` from odef_kernel_time_ms(ctx, 3).  With --baseline the same numbers
the way a user of the library had to take them before: odef_get of the two record fields plus the numpy float64 evaluation of
tests/_errors_reference.py on the host (needs the records in host memory: use --traj 4096).  Prints one JSON line.  Run it in a
process of its own."""
import argparse
import ctypes
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
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    N, ns, d = a.traj, a.nsteps, 3
    tri = d * (d + 1) // 2
    ctx = pkg.Context("lorenz63", 3, host.EK1_ID, N, smooth=True)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-3)
    ctx.solve_fixed(np.arange(ns + 1) * 2.0**-9)
    ctx.smooth()
    # the truth: the smoothed solution itself, shifted by 1e-6 (its values do not matter to the time)
    ptr, nbytes = ctx.device_ptr(host.F_SMOOTH_MEAN)
    ref = torch.empty((ns + 1, d, N), dtype=torch.float64, device="cuda")
    hip = ctypes.CDLL("libamdhip64.so")  # (one strided device-to-device copy of rows 0..d-1 of every record)
    row = d * N * 8
    rc = hip.hipMemcpy2D(ctypes.c_void_p(ref.data_ptr()), ctypes.c_size_t(row), ctypes.c_void_p(ptr), ctypes.c_size_t(ctx.D * N * 8),
                         ctypes.c_size_t(row), ctypes.c_size_t(ns + 1), 3)  # hipMemcpyDeviceToDevice
    assert rc == 0, rc
    ref += 1e-6
    torch.cuda.synchronize()
    ctx.bind_reference(ref.data_ptr(), ref.numel() * 8)
    out = {"traj": N, "n_save": ns + 1, "d": d, "algorithmic_bytes": 8 * N * (ns + 1) * (2 * d + tri)}
    for source in (0, 1):
        best = None
        for _ in range(a.repeat + 1):  # the first request is the warm-up
            ctx.bind_reference(ref.data_ptr(), ref.numel() * 8)  # drops the cache, keeps the records
            t0 = time.perf_counter()
            e = ctx.solution_errors(source)
            wall = (time.perf_counter() - t0) * 1e3
            ms = ctx.kernel_time_ms(3)[0]
            best = ms if best is None else min(best, ms)
        out[f"source{source}_ms"] = round(best, 4)
        out[f"source{source}_wall_ms"] = round(wall, 3)
        out[f"source{source}_fraction_of_8TBps"] = round(out["algorithmic_bytes"] / (best * 1e-3) / 8e12, 4)
        out[f"source{source}_median_chi2"] = float(np.median(e["chi2"]))
    out["kernel"] = ctx.kernel_name(3)
    if a.baseline:
        import _errors_reference as er

        t0 = time.perf_counter()
        mean, cov = ctx.get(host.F_MEAN), ctx.get(host.F_COV_TRIL)
        t1 = time.perf_counter()
        truth = ref.cpu().numpy()
        t2 = time.perf_counter()
        want = er.evaluate(mean, cov, d, truth, dtype=np.float64)
        t3 = time.perf_counter()
        got = ctx.solution_errors(0)
        out["baseline_get_ms"] = round((t1 - t0) * 1e3, 1)
        out["baseline_numpy_ms"] = round((t3 - t2) * 1e3, 1)
        out["baseline_max_rel_diff_l2"] = float(np.abs(want["l2"] - got["l2"]).max() / np.abs(want["l2"]).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
