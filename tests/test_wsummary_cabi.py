"""Weighted ensemble summary without a GPU: the constants in the header, the host layer and the Julia binding; the kernels in the
gfx950 code object of their translation unit; and the host logic that needs no device (`merge_weighted_moments` against the
one-block reference on split synthetic data, the refusal of quantiles together with weights, the new dataclass fields, argument
errors)."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import _wsummary_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
QUANTITIES = ("COUNT", "MEAN", "COV_WITHIN", "COV_BETWEEN", "LOG_EVIDENCE", "ESS")
WANT = {"ODEF_W_BASE": 384, "ODEF_W_LOGWEIGHT": 408}
WANT.update({f"ODEF_W_{src}_{name}": 384 + 8 * s + q for s, src in enumerate(("FILTER", "SMOOTH", "DENSE")) for q, name in enumerate(QUANTITIES)})
NAMES = list(WANT)


def test_wsummary_constants_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 1))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     "  odef_wsummary_field f = ODEF_W_LOGWEIGHT;", "  (void)f;",
                     f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "wsummary.c", tmp_path / "wsummary"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, vals = vals[-1], dict(zip(NAMES, vals[:-1]))
    assert count == 18  # ODEF_F_COUNT_ is unchanged
    assert vals == WANT == host.WSUMMARY_FIELDS
    for s, src_name in enumerate(("FILTER", "SMOOTH", "DENSE")):
        for q, name in enumerate(QUANTITIES):
            assert host.wsummary_field(s, q) == vals[f"ODEF_W_{src_name}_{name}"] == vals["ODEF_W_BASE"] + 8 * s + q
    assert (host.W_COUNT, host.W_MEAN, host.W_COV_WITHIN, host.W_COV_BETWEEN, host.W_LOG_EVIDENCE, host.W_ESS) == tuple(range(6))
    assert host.K_WSUMMARY == 7 and host.W_LOGWEIGHT == vals["ODEF_W_LOGWEIGHT"]
    # distinct from every other family's ids, and none of the other families claims them
    ids = [v for k, v in vals.items() if k != "ODEF_W_BASE"]
    assert len(set(ids)) == len(ids) == 19
    others = set()
    for fam in (host.SUMMARY_FIELDS, host.ERRORS_FIELDS, host.DATA_FIELDS, host.DATA_TIME_FIELDS, host.EVENT_FIELDS, host.QUANTILE_FIELDS):
        others |= set(fam.values())
    others |= set(range(count))
    assert not others & set(ids)
    for f in ids:
        assert not host._is_summary_field(f) and not host._is_errors_field(f) and not host._is_event_field(f)
        assert not host._is_quantile_field(f)
        assert host._is_wsummary_field(f) == (f != vals["ODEF_W_LOGWEIGHT"])
        assert (f in host._DERIVED) == (f != vals["ODEF_W_LOGWEIGHT"])
    for f in others:
        assert not host._is_wsummary_field(f)
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "weighted_ensemble_summary" in jl


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


def test_wsummary_kernels_in_the_code_object(pkg):
    """The six kernels in wsummary.o (the two reductions once per K), and nothing else left out of line there.  A missing object
    or ROCm binutils is a failure, not a skip."""
    pkg.load_library()
    obj = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build", "wsummary.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    syms = _kernel_symbols(obj)
    for name in ("wsummary_max_kernel", "wsummary_weights_kernel", "wsummary_sums_kernel", "wsummary_fold_kernel",
                 "wsummary_centred_kernel", "wsummary_fold_centred_kernel"):
        assert any(name in s for s in syms), (name, syms)
    for name in ("wsummary_sums_kernel", "wsummary_centred_kernel"):
        for k in (1, 2, 4, 8):
            assert any(f"{name}ILi{k}E" in s for s in syms), (name, k, syms)
    assert all("kernel" in s for s in syms), syms


def test_wsummary_field_argument_errors(pkg):
    from odefilters_jl_amd import host

    for source, quantity in ((3, 0), (-1, 0), (0, 6), (0, -1)):
        with pytest.raises(pkg.OdefError, match="no weighted-summary field"):
            host.wsummary_field(source, quantity)
    with pytest.raises(pkg.OdefError, match="no parts"):
        pkg.merge_weighted_moments([])
    four = (np.ones(2, np.int64), np.zeros((2, 2)), np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(pkg.OdefError, match="a part is"):
        pkg.merge_weighted_moments([four])


def _one_block(mean, cov, rc, logw, d):
    r = wr.reference(mean, cov, rc, logw, d)
    return tuple(np.asarray(r[k], np.float64) if k != "count" else r[k] for k in ("count", "mean", "within", "between", "log_evidence", "ess"))


@pytest.mark.parametrize("cuts", [(0, 501, 1001), (0, 1, 400, 401, 1001), (0, 1001)])
def test_merge_weighted_moments_against_the_one_block_reference(pkg, cuts):
    """Shards of synthetic records, each summarised exactly (the reference rounded to float64, every shard with its own shift),
    pool to the reference of the whole within the bounds of one block.  Means of order 1 with a spread of order 1: the limit
    of DESIGN.md 3.12 "Pooling shards" (a spread far below u |m| sqrt(n_r) times the mean) does not apply.  One trajectory is
    dropped by its retcode, one by a NaN weight, one at the last time by a NaN mean; one shard is a single trajectory."""
    rng = np.random.default_rng(len(cuts))
    N, n_t, d, D = 1001, 4, 3, 6
    TRI = D * (D + 1) // 2
    mean = 1.0 + rng.standard_normal((n_t, D, N))
    cov = 1e-3 * rng.standard_normal((n_t, TRI, N))
    rc = np.zeros(N, np.int32)
    rc[7] = 3
    logw = -100.0 - 20.0 * rng.standard_normal(N) ** 2
    logw[600] = np.nan
    logw[0] = -90.0  # the single-trajectory shard carries an ordinary weight
    mean[n_t - 1, 1, 900] = np.nan
    parts = [_one_block(mean[:, :, lo:hi], cov[:, :, lo:hi], rc[lo:hi], logw[lo:hi], d) for lo, hi in zip(cuts[:-1], cuts[1:])]
    got = pkg.merge_weighted_moments(parts)
    ref = wr.reference(mean, cov, rc, logw, d)
    assert ref["count"].tolist() == [N - 2] * (n_t - 1) + [N - 3]
    worst = wr.check(got, ref, d, label=f"{len(parts)} shards")
    print("merge_weighted_moments, worst error / bound:", dict(zip(wr.NAMES, worst)))


def test_merge_weighted_moments_handles_shards_without_mass(pkg):
    rng = np.random.default_rng(3)
    N, n_t, d = 300, 3, 2
    mean = rng.standard_normal((n_t, d, N))
    cov = 1e-3 * rng.standard_normal((n_t, 3, N))
    rc = np.zeros(N, np.int32)
    logw = -50.0 * rng.random(N)
    logw[100:200] = -2000.0  # the middle shard underflows against the others, but not within itself
    mean[0, 0, 200:] = np.nan  # the last shard has nobody at time 0
    logw[:100] = np.where(np.arange(100) == 5, 0.0, -900.0)
    mean[1, 1, 5] = np.inf    # the first shard loses the carrier of its maximum at time 1: Z == 0 there
    cuts = (0, 100, 200, 300)
    parts = [_one_block(mean[:, :, lo:hi], cov[:, :, lo:hi], rc[lo:hi], logw[lo:hi], d) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert parts[0][4][1] == -np.inf and np.isnan(parts[2][4][0]) and parts[2][0][0] == 0
    got = pkg.merge_weighted_moments(parts)
    ref = wr.reference(mean, cov, rc, logw, d)
    wr.check(got, ref, d, label="shards without mass")
    # nobody anywhere, and somebody but no mass anywhere
    empty = tuple(np.full_like(a, np.nan) if a.dtype != np.int64 else np.zeros_like(a) for a in parts[0])
    n, m, w, b, le, ess = pkg.merge_weighted_moments([empty, empty])
    assert np.all(n == 0) and all(np.all(np.isnan(a)) for a in (m, w, b, le, ess))
    massless = (np.full(n_t, 4, np.int64),) + tuple(np.full_like(a, np.nan) for a in parts[0][1:4]) + (np.full(n_t, -np.inf), np.full(n_t, np.nan))
    n, m, w, b, le, ess = pkg.merge_weighted_moments([massless, empty])
    assert np.all(n == 4) and np.all(le == -np.inf) and all(np.all(np.isnan(a)) for a in (m, w, b, ess))


def _moments(n_t=3, d=2):
    tri = d * (d + 1) // 2
    return (np.full(n_t, 5, np.int64), np.arange(n_t * d, dtype=float).reshape(n_t, d), np.ones((n_t, tri)), np.ones((n_t, tri)))


def test_summary_dataclass_has_no_weights_unless_asked(pkg):
    s = pkg.EnsembleSummary.from_moments([0.0, 1.0, 2.0], *_moments())
    assert s.ess is None and s.log_evidence is None and s.med is None
    le, ess = np.array([-1.0, -2.0, -3.0]), np.array([2.0, 3.0, 4.0])
    s = pkg.EnsembleSummary.from_moments([0.0, 1.0, 2.0], *_moments(), le, ess)
    assert s.ess is ess and s.log_evidence is le and s.cov.shape == (3, 2, 2)


def _stub_solution(pkg, shard=None):
    moments = _moments()
    weighted = moments + (np.array([-1.0, -2.0, -3.0]), np.array([2.0, 3.0, 4.0]))
    seen = []

    class Ctx:
        N = 5
        ensemble_moments = staticmethod(lambda source: moments)

        @staticmethod
        def weighted_moments(source, log_weights=None):
            seen.append((source, log_weights))
            return weighted

    class StubSolution(pkg.EnsembleSolution):  # a solve needs a GPU; the context is stood in for by its two summary methods
        def __init__(self):
            self.shard, self.adaptive = shard, False
            self.ctx = Ctx()

        smoothed = True
        t = np.arange(3, dtype=float)

    return StubSolution(), weighted, seen


def test_summary_with_log_weights_builds_the_weighted_summary(pkg):
    sol, weighted, seen = _stub_solution(pkg)
    assert sol.summary().ess is None and not seen  # without weights: the unweighted path, untouched
    logw = np.linspace(-3.0, 0.0, 5)
    s = sol.summary(log_weights=logw)
    assert seen[-1][0] == 1 and np.array_equal(seen[-1][1], logw)  # the smoothed records of a smoothed solution
    assert s.ess is weighted[5] and s.log_evidence is weighted[4] and np.array_equal(s.mean, weighted[1])
    assert sol.summary(smoothed=False, log_weights=logw).n is weighted[0] and seen[-1][0] == 0
    with pytest.raises(pkg.OdefError, match="weighted quantiles are not built"):
        sol.summary(quantiles=(0.05, 0.95), log_weights=logw)
    sol.adaptive = True
    with pytest.raises(pkg.OdefError, match=r"summary\(\): an adaptive solve"):
        sol.summary(log_weights=logw)
