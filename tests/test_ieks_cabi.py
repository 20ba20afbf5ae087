"""IEKS at the C ABI and in the host layer, without a GPU: the new enum value and field in the header, the host constants
and the Julia binding; the IEKS kernels in the library's gfx950 code objects for every compiled-in field of d <= 10; and the
refusals that happen before any device is touched (odef_create's argument checks, the host's solve_ieks / IEKS checks)."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import tempfile
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LANE_FIELDS = {"fhn": ("RhsFHN", 2), "lorenz63": ("RhsLorenz63", 3), "lotka_volterra": ("RhsLotkaVolterra", 2),
               "vanderpol": ("RhsVanDerPol", 2), "linear": ("RhsLinear", 2)}


def test_enum_and_field_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     '  printf("%d %d %d\\n", (int)ODEF_IEKS, (int)ODEF_F_LINEARIZE_AT, (int)ODEF_F_COUNT_);', "  return 0;", "}"])
    cfile, exe = tmp_path / "ieks.c", tmp_path / "ieks"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    ieks, lin, count = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (ieks, lin, count) == (2, 17, 18)
    assert host.IEKS_ID == ieks and host.F_LINEARIZE_AT == host.ODEF_F_LINEARIZE_AT == lin
    assert pkg.IEKS._id == ieks
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    assert re.search(r"ODEF_IEKS = (\d+)", jl).group(1) == "2"
    assert re.search(r"F_LINEARIZE_AT = (\d+)", jl).group(1) == "17"
    assert "solve_ieks" in jl


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


@pytest.mark.parametrize("field", sorted(LANE_FIELDS))
def test_ieks_kernels_in_the_code_objects(pkg, field):
    """ek_filter_fixed_ieks_kernel<RHS, q, LAG> for every order and both LAG, ek_filter_rows_ieks_kernel<RHS, q> for every order
    with d(q+1) <= 16, in the field's translation unit.  A missing object or ROCm binutils is a failure, not a skip."""
    pkg.load_library()  # (built by the session's build())
    obj = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build", f"inst_{field}.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    rhs, d = LANE_FIELDS[field]
    syms = _kernel_symbols(obj)
    lane = [s for s in syms if "ek_filter_fixed_ieks_kernel" in s and rhs in s]
    rows = [s for s in syms if "ek_filter_rows_ieks_kernel" in s and rhs in s]
    for q in range(1, 6):
        for lag in ("1", "0"):
            assert any(f"{rhs}ELi{q}ELb{lag}E" in s for s in lane), (field, q, lag, lane)
        assert any(f"{rhs}ELi{q}EE" in s for s in rows) == (d * (q + 1) <= 16), (field, q, rows)
    # the EK1 kernels are still there under their own names
    assert any("ek_filter_fixed_kernel" in s and rhs in s for s in syms)


def _cfg(host, **kw):
    cfg = host.OdefConfig(struct_size=C.sizeof(host.OdefConfig), alg=host.IEKS_ID, order=3, diffusion=0, smooth=1, rhs_id=1, d=3,
                          n_params=3, params_shared=1, save_mode=1, device=-1, want_loglik=1, n_traj=64)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("kw,msg", [
    (dict(smooth=0), b"IEKS always smooths"),
    (dict(diffusion=3, alg=2), b"MV diffusion models require EK0"),
    (dict(diffusion=4, alg=2), b"MV diffusion models require EK0"),
    (dict(rhs_id=5, d=28, n_params=0, order=2), b"IEKS runs on the lane kernels only"),
    (dict(rhs_id=6, d=16, n_params=1, order=2), b"IEKS runs on the lane kernels only"),
])
def test_create_refusals(pkg, kw, msg):
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    h = C.c_void_p()
    assert lib.odef_create(C.byref(h), C.byref(_cfg(host, **kw))) != 0
    assert msg in lib.odef_last_error(None)


def _fake_solution(pkg, order=3, diffusionmodel="dynamic", smooth=True, prior="ibm", N=8):
    sol = pkg.EnsembleSolution.__new__(pkg.EnsembleSolution)
    sol.alg = types.SimpleNamespace(prior=prior, order=order, diffusionmodel=diffusionmodel, smooth=smooth)
    sol.ctx = types.SimpleNamespace(N=N)
    sol.adaptive = False
    return sol


def test_host_refusals(pkg):
    prob = pkg.ODEProblem("lorenz63", [1.0, 0.0, 0.0], (0.0, 1.0), (10.0, 28.0, 8.0 / 3.0))
    with pytest.raises(pkg.OdefError, match="fixed grids"):
        pkg.solve_ieks(prob, pkg.IEKS(order=3), adaptive=True, dt=0.01)
    with pytest.raises(pkg.OdefError, match="fixed grids"):
        pkg.solve_ieks(prob, pkg.IEKS(order=3), dt=0.01)  # solve's default is adaptive
    with pytest.raises(pkg.OdefError, match="MV diffusion models require EK0"):
        pkg.solve_ieks(prob, pkg.IEKS(order=3, diffusionmodel="dynamicMV"), adaptive=False, dt=0.01)
    with pytest.raises(pkg.OdefError, match="iterations"):
        pkg.solve_ieks(prob, pkg.IEKS(order=3), adaptive=False, dt=0.01, iterations=0)
    # IEKS(linearize_at = sol): the reference's assertions (src/ieks.jl:32-38)
    ok = _fake_solution(pkg)
    assert pkg.IEKS(order=3, linearize_at=ok).linearize_at is ok
    for bad in (_fake_solution(pkg, order=2), _fake_solution(pkg, diffusionmodel="fixed"), _fake_solution(pkg, smooth=False),
                _fake_solution(pkg, prior="ioup")):
        with pytest.raises(AssertionError):
            pkg.IEKS(order=3, linearize_at=bad)
    with pytest.raises(AssertionError):
        pkg.IEKS(order=3, linearize_at="not a solution")
    # ... plus the same ensemble size, and fixed grids
    ens = pkg.EnsembleProblem(prob, perturb_scale=1e-2)
    with pytest.raises(pkg.OdefError, match="trajectories"):
        pkg.solve(ens, pkg.IEKS(order=3, linearize_at=ok), trajectories=16, adaptive=False, dt=0.01)
    with pytest.raises(pkg.OdefError, match="fixed grids"):
        pkg.solve(ens, pkg.IEKS(order=3, linearize_at=ok), trajectories=8, adaptive=True)
