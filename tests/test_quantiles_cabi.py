"""Ensemble quantiles without a GPU: the constants in the header, the host layer and the Julia binding; the kernels in the gfx950
code object of their translation unit; and the host logic that needs no device (argument errors, the new dataclass fields, the
refusal for sharded solves, `summary()` without quantiles on a context that has `ensemble_moments` only)."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
WANT = {
    "ODEF_Q_BASE": 320, "ODEF_Q_FILTER": 320, "ODEF_Q_COUNT_FILTER": 321, "ODEF_Q_SMOOTH": 328, "ODEF_Q_COUNT_SMOOTH": 329,
    "ODEF_Q_DENSE": 336, "ODEF_Q_COUNT_DENSE": 337, "ODEF_Q_PROBS": 344,
}
NAMES = list(WANT)


def test_quantile_constants_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 1))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     "  odef_quantile_field f = ODEF_Q_PROBS;", "  (void)f;",
                     f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "quantiles.c", tmp_path / "quantiles"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, vals = vals[-1], dict(zip(NAMES, vals[:-1]))
    assert count == 18
    assert vals == WANT == host.QUANTILE_FIELDS
    for s, src_name in enumerate(("FILTER", "SMOOTH", "DENSE")):
        assert host.quantile_field(s, 0) == vals[f"ODEF_Q_{src_name}"] == vals["ODEF_Q_BASE"] + 8 * s
        assert host.quantile_field(s, 1) == vals[f"ODEF_Q_COUNT_{src_name}"] == vals["ODEF_Q_BASE"] + 8 * s + 1
    assert host.K_QUANTILES == 6
    # distinct from every other family's ids, and none of the other families claims them
    ids = [v for k, v in vals.items() if k != "ODEF_Q_BASE"]
    assert len(set(ids)) == len(ids) == 7
    others = set()
    for fam in (host.SUMMARY_FIELDS, host.ERRORS_FIELDS, host.DATA_FIELDS, host.DATA_TIME_FIELDS, host.EVENT_FIELDS):
        others |= set(fam.values())
    others |= set(range(count))
    assert not others & set(ids)
    for f in ids:
        assert not host._is_summary_field(f) and not host._is_errors_field(f) and not host._is_event_field(f)
        assert host._is_quantile_field(f) == (f != vals["ODEF_Q_PROBS"])
    for f in others:
        assert not host._is_quantile_field(f)
    for f in ids[:-1]:
        assert f in host._DERIVED
    # the summary's constants are as they were
    assert host.SUMMARY_FIELDS == {
        "ODEF_S_BASE": 64,
        "ODEF_S_FILTER_COUNT": 64, "ODEF_S_FILTER_MEAN": 65, "ODEF_S_FILTER_COV_WITHIN": 66, "ODEF_S_FILTER_COV_BETWEEN": 67,
        "ODEF_S_SMOOTH_COUNT": 72, "ODEF_S_SMOOTH_MEAN": 73, "ODEF_S_SMOOTH_COV_WITHIN": 74, "ODEF_S_SMOOTH_COV_BETWEEN": 75,
        "ODEF_S_DENSE_COUNT": 80, "ODEF_S_DENSE_MEAN": 81, "ODEF_S_DENSE_COV_WITHIN": 82, "ODEF_S_DENSE_COV_BETWEEN": 83,
    }
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "ensemble_quantiles" in jl


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


def test_quantile_kernels_in_the_code_object(pkg):
    """The six kernels in quantiles.o, and nothing else left out of line there.  A missing object or ROCm binutils is a failure,
    not a skip."""
    pkg.load_library()
    obj = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build", "quantiles.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    syms = _kernel_symbols(obj)
    for name in ("quantile_init_kernel", "quantile_mask_kernel", "quantile_start_kernel", "quantile_hist_kernel",
                 "quantile_select_kernel", "quantile_finish_kernel"):
        assert any(name in s for s in syms), (name, syms)
    assert all("kernel" in s for s in syms), syms


def test_quantile_field_argument_errors(pkg):
    from odefilters_jl_amd import host

    for source, quantity in ((3, 0), (-1, 0), (0, 2), (0, -1)):
        with pytest.raises(pkg.OdefError, match="no ensemble-quantile field"):
            host.quantile_field(source, quantity)


def _moments(n_t=3, d=2):
    tri = d * (d + 1) // 2
    return (np.full(n_t, 5, np.int64), np.arange(n_t * d, dtype=float).reshape(n_t, d), np.ones((n_t, tri)), np.ones((n_t, tri)))


def test_summary_dataclass_has_no_quantiles_unless_asked(pkg):
    s = pkg.EnsembleSummary.from_moments([0.0, 1.0, 2.0], *_moments())
    assert s.med is None and s.qlow is None and s.qhigh is None and s.quantile_probs is None
    assert s.mean.shape == (3, 2) and s.cov.shape == (3, 2, 2)


def _stub_solution(pkg, shard):
    moments = _moments()

    class StubSolution(pkg.EnsembleSolution):  # a solve needs a GPU; the context is stood in for by its one summary method
        def __init__(self):
            self.shard, self.adaptive = shard, False
            self.ctx = type("Ctx", (), {"ensemble_moments": staticmethod(lambda source: moments)})()

        smoothed = False
        t = np.arange(3, dtype=float)

    return StubSolution(), moments


def test_summary_without_quantiles_touches_ensemble_moments_only(pkg):
    sol, moments = _stub_solution(pkg, None)
    s = sol.summary()
    np.testing.assert_array_equal(s.mean, moments[1])
    assert s.med is None and s.quantile_probs is None
    with pytest.raises(AttributeError):  # the stub has no quantile pass: asking for one reaches for it
        sol.summary(quantiles=(0.05, 0.95))


def test_sharded_solutions_refuse_quantiles(pkg):
    sol, _ = _stub_solution(pkg, (0, 500, 1001, 2))
    with pytest.raises(pkg.OdefError, match="do not pool"):
        sol.quantiles([0.5])
    with pytest.raises(pkg.OdefError, match="do not pool"):
        sol.summary(quantiles=(0.05, 0.95))
    one, moments = _stub_solution(pkg, (0, 1001, 1001, 1))  # a world of one is no sharding: only the stub's missing pass stops it
    with pytest.raises(AttributeError):
        one.quantiles([0.5])
