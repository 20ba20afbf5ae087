"""The weighted ensemble summary of a distributed solve without a GPU: two ranks over gloo, every rank's device reduction stood
in for by the extended-precision reference of its block.  Covers `dist.allgather_weighted_moments` (one collective, the packing
offsets), the cut of whole-ensemble `log_weights` to the rank's block in `EnsembleSolution.summary(log_weights=...)`, a torch
tensor cut the same way, and the pooling; and the world-of-one path."""
import multiprocessing as mp
import os
import socket

import numpy as np

import _wsummary_reference as wr

KEYS = ("count", "mean", "within", "between", "log_evidence", "ess")


def _ensemble(n_t=4, N=1001, d=3, D=6):
    rng = np.random.default_rng(19)
    mean = 1.0 + rng.standard_normal((n_t, D, N))
    cov = 1e-3 * rng.standard_normal((n_t, D * (D + 1) // 2, N))
    rc = np.zeros(N, np.int32)
    rc[7] = 3
    logw = -100.0 - 20.0 * rng.standard_normal(N) ** 2
    logw[600] = np.nan
    mean[n_t - 1, 1, 900] = np.nan
    return mean, cov, rc, logw, d


def _block(mean, cov, rc, logw, d):
    r = wr.reference(mean, cov, rc, logw, d)
    return tuple(r[k] if k == "count" else np.asarray(r[k], np.float64) for k in KEYS)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch
    import torch.distributed as td

    import odefilters_jl_amd as pkg
    from odefilters_jl_amd import dist as od

    od.init_from_env(backend="gloo")
    mean, cov, rc, logw, d = _ensemble()
    N = mean.shape[2]
    lo, hi = od.shard_bounds(N, rank, world)

    calls = []
    real = td.all_gather_into_tensor

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    td.all_gather_into_tensor = counting
    seen = []

    class Ctx:  # the solve needs a GPU; the shard's device reduction is the reference of the block under the weights it is handed
        N = hi - lo

        @staticmethod
        def weighted_moments(source, log_weights=None):
            seen.append(np.array(log_weights))
            return _block(mean[:, :, lo:hi], cov[:, :, lo:hi], rc[lo:hi], log_weights, d)

    class ShardSolution(pkg.EnsembleSolution):
        def __init__(self):
            self.shard, self.adaptive = (lo, hi, N, world), False
            self.ctx = Ctx()

        smoothed = False
        t = np.arange(mean.shape[0], dtype=float)

    sol = ShardSolution()
    s = sol.summary(log_weights=logw)                      # the whole ensemble's weights: cut to the block
    cut_ok = np.array_equal(seen[-1], logw[lo:hi], equal_nan=True)
    s2 = sol.summary(log_weights=torch.from_numpy(logw))   # a tensor is cut the same way
    cut_ok = cut_ok and np.array_equal(seen[-1], logw[lo:hi], equal_nan=True)
    s3 = sol.summary(log_weights=logw[lo:hi])              # the rank's own block is taken as it is
    cut_ok = cut_ok and np.array_equal(seen[-1], logw[lo:hi], equal_nan=True)
    same = all(np.array_equal(getattr(s, k), getattr(o, k), equal_nan=True) for o in (s2, s3)
               for k in ("n", "mean", "cov_within", "cov_between", "log_evidence", "ess"))
    q.put((rank, len(calls), cut_ok, same, s.n, s.mean, s.cov_within, s.cov_between, s.log_evidence, s.ess))
    td.barrier()
    td.destroy_process_group()
    del torch


def test_two_rank_weighted_summary_is_that_of_the_whole_ensemble(pkg):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        item = q.get(timeout=180)
        got[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    mean, cov, rc, logw, d = _ensemble()
    want = wr.reference(mean, cov, rc, logw, d)
    il = np.tril_indices(d)
    for r in range(world):
        calls, cut_ok, same, n, m, w, b, le, ess = got[r]
        assert calls == 3 and cut_ok and same  # one collective per summary
        wr.check((n, m, w[:, il[0], il[1]], b[:, il[0], il[1]], le, ess), want, d, label=f"rank {r}")
    for a, b in zip(got[0][3:], got[1][3:]):
        np.testing.assert_array_equal(a, b)


def test_a_world_of_one_returns_its_block():
    from odefilters_jl_amd import dist as od

    mean, cov, rc, logw, d = _ensemble(n_t=2)
    block = _block(mean, cov, rc, logw, d)
    out = od.allgather_weighted_moments(block, 1)
    assert len(out) == 1 and all(a is b for a, b in zip(out[0], block))
