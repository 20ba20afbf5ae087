"""Ensemble sharding across GPUs: one process per GPU (torchrun), contiguous blocks of the
trajectory index per rank, no exchange while stepping (trajectories are independent), one
all-gather of the per-shard results at the end (`torch.distributed` backend "nccl" = RCCL
over xGMI on ROCm; "gloo" on CPU for tests).  SURVEY.md 8(e)."""
from __future__ import annotations

import os
from typing import Tuple

import torch
import torch.distributed as dist


def shard_bounds(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block [lo, hi) of rank `rank`; the first `total % world` ranks get one extra.  The arithmetic is the
    C ABI's (`odef_shard_range`, include/odefilter.h), so the one-process-per-GPU path here and the single-process
    `odef_group` a Julia host drives cut an ensemble identically."""
    from .host import shard_range

    lo, n = shard_range(total, world, rank)
    return lo, lo + n


def init_from_env(backend: str = "nccl") -> Tuple[int, int, int]:
    """(rank, world, local_rank) from torchrun's environment; initialises the process group when world > 1."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def allgather_shards(local: torch.Tensor, world: int) -> torch.Tensor:
    """The single collective of the path: gathers equally sized per-rank result blocks
    [..., n_local] into [world, ..., n_local]."""
    if world == 1:
        return local.unsqueeze(0)
    flat = local.contiguous().view(-1)
    out = torch.empty(world * flat.numel(), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, flat)  # 1-D concat form: accepted by both RCCL and gloo
    return out.view((world,) + tuple(local.shape))


def gathered_to_global(g: torch.Tensor) -> torch.Tensor:
    """[world, K, n_local] -> [K, world*n_local] in global trajectory order."""
    w, k, n = g.shape
    return g.permute(1, 0, 2).reshape(k, w * n)


def allgather_moments(moments, world: int):
    """One all_gather of a rank's ensemble-summary block (count [n_t], mean [n_t, d], within and between [n_t, tri]; a few
    kilobytes, so host memory and any backend): the list of every rank's (count, mean, within, between), in rank order, for
    `host.merge_moments`.  Counts travel as doubles (exact below 2^53).  With the "nccl" backend the block goes through the
    rank's current GPU, since RCCL moves device memory only."""
    import numpy as np

    n, m, w, b = moments
    if world == 1:
        return [moments]
    n_t, d, tri = m.shape[0], m.shape[1], w.shape[1]
    flat = np.concatenate([np.asarray(n, float).reshape(n_t, 1), m, w, b], axis=1)  # [n_t, 1 + d + 2 tri]
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    g = allgather_shards(torch.from_numpy(np.ascontiguousarray(flat)).to(dev), world).cpu().numpy()
    return [(g[r, :, 0].astype(np.int64), g[r, :, 1:1 + d], g[r, :, 1 + d:1 + d + tri], g[r, :, 1 + d + tri:]) for r in range(world)]


def allgather_weighted_moments(moments, world: int):
    """`allgather_moments` for a rank's weighted-summary block (count, mean, within, between, log_evidence, ess): the list of
    every rank's six arrays, in rank order, for `host.merge_weighted_moments`."""
    import numpy as np

    n, m, w, b, le, ess = moments
    if world == 1:
        return [moments]
    n_t, d, tri = m.shape[0], m.shape[1], w.shape[1]
    flat = np.concatenate([np.asarray(n, float).reshape(n_t, 1), m, w, b, np.asarray(le, float).reshape(n_t, 1),
                           np.asarray(ess, float).reshape(n_t, 1)], axis=1)  # [n_t, 3 + d + 2 tri]
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    g = allgather_shards(torch.from_numpy(np.ascontiguousarray(flat)).to(dev), world).cpu().numpy()
    o = 1 + d + 2 * tri
    return [(g[r, :, 0].astype(np.int64), g[r, :, 1:1 + d], g[r, :, 1 + d:1 + d + tri], g[r, :, 1 + d + tri:o], g[r, :, o], g[r, :, o + 1])
            for r in range(world)]
