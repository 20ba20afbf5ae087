#!/usr/bin/env python3
"""Interleaved A/B of a launch-time knob of the fixed-step lane filter on the bench workload, within one process on one box.

Lorenz-63 EK1(3), fixed dt = 2^-9, every step saved, want_loglik on, MEAN and COV_TRIL bound to torch-owned buffers as bench.py
binds them.  Per round the filter runs once under every value of --values in turn (default "0,1,0": A, B and A again, so that
the A/A pair gives the noise floor of the same rounds); the time is odef_kernel_time_ms(ctx, 0).  One JSON line per round,
then one summary line: median and minimum per position, the gain of every position over the first, and for values that occur
twice the A/A spread (difference of the two medians, and the median of the round-wise differences).

    python tools/wave_map_ab.py                                   # ODEF_WAVE_MAP 0 / 1 / 0 at 65 536 x 1 024
    python tools/wave_map_ab.py --traj 16384 --env ODEF_FILTER_ROWS_MAX_N=0 --knob ODEF_FILTER_LAG_MAX_N --values 0,1000000000,0
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traj", type=int, default=65536)
    ap.add_argument("--nsteps", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--knob", default="ODEF_WAVE_MAP")
    ap.add_argument("--values", default="0,1,0")
    ap.add_argument("--env", action="append", default=[], metavar="NAME=VALUE", help="set for the whole run")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    for kv in args.env:
        k, v = kv.split("=", 1)
        os.environ[k] = v
    values = args.values.split(",")

    import torch

    import odefilters_jl_amd as pkg

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    N, q, D = args.traj, 3, 12
    TRI = D * (D + 1) // 2
    n_save = args.nsteps + 1
    tgrid = np.arange(n_save) * 2.0**-9
    ctx = pkg.Context("lorenz63", q, 1, N, save_everystep=True, smooth=False, device=0, want_loglik=True)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    mean = torch.empty((n_save, D, N), dtype=torch.float64, device=dev)
    cov = torch.empty((n_save, TRI, N), dtype=torch.float64, device=dev)
    ctx.bind_device(0, mean.data_ptr(), mean.numel() * 8)
    ctx.bind_device(1, cov.data_ptr(), cov.numel() * 8)
    ctx.set_problem_perturbed([1.0, 0.0, 0.0], [10.0, 28.0, 8.0 / 3.0], 0.0, 1e-2)

    def once(v):
        os.environ[args.knob] = v  # the launcher reads it at every launch
        ctx.solve_fixed(tgrid)
        return ctx.kernel_time_ms(0)[0], ctx.kernel_name(0)

    head = {"tag": args.tag, "knob": args.knob, "values": values, "traj": N, "nsteps": args.nsteps, "env": args.env,
            "device": torch.cuda.get_device_name(0), "host": os.uname().nodename}
    kernels = []
    for v in values * 2:  # warm-up: first touch of the records, code objects of every kernel the values select
        kernels.append(once(v)[1])
    head["kernels"] = kernels[: len(values)]
    print(json.dumps(head), flush=True)
    ms = [[] for _ in values]
    for r in range(args.rounds):
        row = [once(v)[0] for v in values]
        for k, t in enumerate(row):
            ms[k].append(t)
        print(json.dumps({"tag": args.tag, "round": r, "knob": args.knob, "values": values, "kernel_ms": row}), flush=True)
    assert bool(torch.isfinite(mean[n_save - 1]).all().item()) and bool((ctx.get(10) == 0).all())
    ms = np.array(ms)
    med, mn = np.median(ms, axis=1), ms.min(axis=1)
    out = {"tag": args.tag, "summary": True, "knob": args.knob, "values": values, "traj": N, "rounds": args.rounds,
           "median_ms": med.tolist(), "min_ms": mn.tolist(),
           "median_gain_over_first": ((med[0] - med) / med[0]).tolist()}
    same = [(i, j) for i in range(len(values)) for j in range(i + 1, len(values)) if values[i] == values[j]]
    if same:
        i, j = same[0]
        out["aa_positions"] = [i, j]
        out["aa_spread_of_medians"] = float(abs(med[i] - med[j]) / med[i])
        out["aa_median_roundwise_abs_diff"] = float(np.median(np.abs(ms[i] - ms[j])) / med[i])
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
