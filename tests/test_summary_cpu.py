"""Ensemble summary without a GPU: the new constants in the header, the host layer and the Julia binding; the reduction
kernels in the gfx950 code object of their translation unit; `merge_moments` against the extended-precision reference on a
sharded random ensemble; and the distributed summary over gloo (two ranks, one collective)."""
import glob
import os
import re
import shutil
import socket
import subprocess
import tempfile

import numpy as np
import torch.multiprocessing as mp

import _summary_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = ["ODEF_S_BASE"] + [f"ODEF_S_{src}_{q}" for src in ("FILTER", "SMOOTH", "DENSE")
                           for q in ("COUNT", "MEAN", "COV_WITHIN", "COV_BETWEEN")]


def test_summary_constants_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 1))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     "  odef_summary_field f = ODEF_S_DENSE_COV_BETWEEN;", "  (void)f;",
                     f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "summary.c", tmp_path / "summary"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, vals = vals[-1], dict(zip(NAMES, vals[:-1]))
    assert count == 18
    assert all(v >= count for v in vals.values())
    ids = [v for k, v in vals.items() if k != "ODEF_S_BASE"]
    assert len(set(ids)) == len(ids) == 12
    assert vals == host.SUMMARY_FIELDS
    for s, src_name in enumerate(("FILTER", "SMOOTH", "DENSE")):
        for q, q_name in enumerate(("COUNT", "MEAN", "COV_WITHIN", "COV_BETWEEN")):
            assert host.summary_field(s, q) == vals[f"ODEF_S_{src_name}_{q_name}"] == vals["ODEF_S_BASE"] + 8 * s + q
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "ensemble_summary" in jl and "merge_moments" in jl


def _kernel_symbols(obj):
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        cos = [f for f in glob.glob(local + ".*") if "amdgcn" in f and "gfx950" in f]
        assert cos, f"no gfx950 code object in {obj}"
        out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", cos[0]], check=True, capture_output=True, text=True).stdout
    return [ln.split()[7] for ln in out.splitlines() if len(ln.split()) >= 8 and ln.split()[3] == "FUNC"]


def test_summary_kernels_in_the_code_object(pkg):
    """summary_sums_kernel<K> and summary_centred_kernel<K> for K = 1, 2, 4, 8 and the fold kernel, in summary.o, and nothing
    else left out of line there.  A missing object or ROCm binutils is a failure, not a skip."""
    pkg.load_library()
    obj = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build", "summary.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    syms = _kernel_symbols(obj)
    for k in (1, 2, 4, 8):
        assert any("summary_sums_kernel" in s and f"ILi{k}E" in s for s in syms), (k, syms)
        assert any("summary_centred_kernel" in s and f"ILi{k}E" in s for s in syms), (k, syms)
    assert any("summary_fold_kernel" in s for s in syms)
    assert all("kernel" in s for s in syms), syms


def _random_ensemble(n_t=5, d=3, N=1001, seed=3):
    """Values of size <= 2 with a spread of 1e-2 .. 1e-1.  The range is chosen for the MERGED covariance of the means, whose bound
    n u sqrt(B_kk B_ll) a pooled result can only meet when the spread is not too small: a shard hands over its mean m_r rounded to
    float64 (error <= u |m|), the pooled term n_r (m_r - m)(m_r - m)' / n carries 2 |m_r - m| u |m| of it, and with
    |m_r - m| ~ 3 sigma / sqrt(n_r) for both means that is about 24 sigma u |m| / sqrt(n_r) = 4.3 sigma u at |m| = 2, n_r = 125
    (eight shards) -- below n u sigma^2 = 1001 u sigma^2 for sigma >= 1e-2 by a factor 2 or more.  Below sigma ~ 2 |m| / (n
    sqrt(n_r)) no combination of float64 blocks can meet that bound; one context's own summary is not affected,
    it centres on the device."""
    rng = np.random.default_rng(seed)
    D, T = d + 2, (d + 2) * (d + 3) // 2
    centre = rng.uniform(-2.0, 2.0, size=(n_t, D, 1))
    spread = 10.0 ** rng.uniform(-2, -1, size=(n_t, 1, 1))
    mean = centre + spread * rng.standard_normal((n_t, D, N))
    cov = rng.uniform(-1e-6, 1e-6, size=(n_t, T, N))
    rc = np.zeros(N, np.int32)
    rc[417] = 3                  # one trajectory excluded by its retcode
    mean[2, 1, 5] = np.nan       # and one at one time only
    return mean, cov, rc, d


def test_merge_moments_equals_the_whole_ensemble_reference(pkg):
    mean, cov, rc, d = _random_ensemble()
    N = mean.shape[2]
    whole = sr.reference(mean, cov, rc, d)
    assert whole[0].tolist() == [N - 1, N - 1, N - 2, N - 1, N - 1]
    for world in (1, 2, 3, 8):
        bounds = sr.shard_bounds(N, world)
        parts = []
        for r, (lo, hi) in enumerate(bounds):
            rc_r = rc[lo:hi].copy()
            if world == 3 and r == 1:
                continue  # (checked below: an empty shard)
            ref = sr.reference(mean[:, :, lo:hi], cov[:, :, lo:hi], rc_r, d)
            parts.append(tuple(np.asarray(a, np.float64) if k else a for k, a in enumerate(ref[:4])))
        if world == 3:  # one shard made empty: every trajectory of it excluded, so the whole-ensemble reference drops it too
            lo, hi = bounds[1]
            rc2 = rc.copy()
            rc2[lo:hi] = 1
            ref = sr.reference(mean[:, :, lo:hi], cov[:, :, lo:hi], rc2[lo:hi], d)
            assert np.all(ref[0] == 0)
            parts.insert(1, tuple(np.asarray(a, np.float64) if k else a for k, a in enumerate(ref[:4])))
            want = sr.reference(mean, cov, rc2, d)
        else:
            want = whole
        got = pkg.merge_moments(parts)
        sr.check(got, want, d, label=f"world {world}")
    # all shards empty at every time: NaN moments
    rc3 = np.ones(N, np.int32)
    ref = sr.reference(mean, cov, rc3, d)
    n, m, w, b = pkg.merge_moments([tuple(np.asarray(a, np.float64) if k else a for k, a in enumerate(ref[:4]))] * 2)
    assert np.all(n == 0) and np.all(np.isnan(m)) and np.all(np.isnan(w)) and np.all(np.isnan(b))


def test_summary_dataclass_unpacks_and_adds(pkg):
    mean, cov, rc, d = _random_ensemble(n_t=3)
    rc[:] = 0
    n, m, w, b = (np.asarray(a, np.float64) if k else a for k, a in enumerate(sr.reference(mean, cov, rc, d)[:4]))
    s = pkg.EnsembleSummary.from_moments([0.0, 1.0, 2.0], n, m, w, b)
    assert s.cov.shape == (3, d, d) and s.std.shape == (3, d)
    np.testing.assert_array_equal(s.cov, s.cov_within + s.cov_between)
    np.testing.assert_array_equal(s.cov_between[:, 2, 1], b[:, 4])
    np.testing.assert_array_equal(s.cov_between[:, 1, 2], b[:, 4])
    np.testing.assert_allclose(s.std ** 2, np.diagonal(s.cov, axis1=1, axis2=2), rtol=1e-15)


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
    import _summary_reference as ref_mod

    od.init_from_env(backend="gloo")
    mean, cov, rc, d = _random_ensemble()
    N = mean.shape[2]
    lo, hi = od.shard_bounds(N, rank, world)
    local = ref_mod.reference(mean[:, :, lo:hi], cov[:, :, lo:hi], rc[lo:hi], d)
    moments = tuple(np.asarray(a, np.float64) if k else a for k, a in enumerate(local[:4]))

    calls = []
    real = td.all_gather_into_tensor

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    td.all_gather_into_tensor = counting

    class ShardSolution(pkg.EnsembleSolution):  # the solve itself needs a GPU; the shard's device reduction is stood in for
        def __init__(self):
            self.shard, self.adaptive = (lo, hi, N, world), False
            self.ctx = type("Ctx", (), {"ensemble_moments": staticmethod(lambda source: moments)})()

        smoothed = False
        t = np.arange(mean.shape[0], dtype=float)

    s = ShardSolution().summary()
    q.put((rank, len(calls), s.n, s.mean, s.cov_within, s.cov_between))
    td.barrier()
    td.destroy_process_group()
    del torch


def test_two_rank_summary_is_the_whole_ensemble_summary_from_one_collective(pkg):
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
    mean, cov, rc, d = _random_ensemble()
    want = sr.reference(mean, cov, rc, d)
    il = np.tril_indices(d)
    for r in range(world):
        calls, n, m, w, b = got[r]
        assert calls == 1
        sr.check((n, m, w[:, il[0], il[1]], b[:, il[0], il[1]]), want, d, label=f"rank {r}")
    for a, b in zip(got[0][1:], got[1][1:]):
        np.testing.assert_array_equal(a, b)
