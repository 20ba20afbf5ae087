"""Time-dependent fields f(u, p, t) at the C ABI, without a GPU: the compiled-in field ODEF_RHS_FORCED in the header, the host
constants and the Julia binding; its kernels in the library's gfx950 code objects; run-time compiled `has_time` structs through
odef_rhs_compile (which cross-compiles); and the refusal of a shape that would need the workgroup-per-trajectory kernels."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


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

FORCED_F = """
  static constexpr int d = 2, np = 3;
  static constexpr bool has_time = true;
  template <class T>
  __device__ static void f(const T (&u)[2], const double* p, T t, T (&du)[2]) {
    du[0] = p[0] * u[0] + p[1] * t;
    du[1] = p[2] * t * u[1];
  }
"""
FORCED_JAC = """
  __device__ static void jac(const double (&u)[2], const double* p, double t, double (&J)[2][2]) {
    J[0][0] = p[0]; J[0][1] = 0.0; J[1][0] = 0.0; J[1][1] = p[2] * t;
  }
"""


def _cfg(host, **kw):
    cfg = host.OdefConfig(struct_size=C.sizeof(host.OdefConfig), alg=1, order=3, diffusion=0, smooth=1, rhs_id=7, d=2,
                          n_params=3, params_shared=1, save_mode=1, device=-1, want_loglik=1, n_traj=64)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_forced_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     '  printf("%d\\n", (int)ODEF_RHS_FORCED);', "  return 0;", "}"])
    cfile, exe = tmp_path / "forced.c", tmp_path / "forced"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == 7
    assert host.RHS["forced"] == 7 and host.RHS_DIMS["forced"] == (2, 3)
    assert re.search(r":forced => (\d+)", open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()).group(1) == "7"


def test_create_accepts_the_forced_field(pkg):
    """Every argument check passes for rhs_id = 7; without a device odef_create then stops at the device, not at the id."""
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    h = C.c_void_p()
    rc = lib.odef_create(C.byref(h), C.byref(_cfg(host)))
    if rc == 0:
        lib.odef_destroy(h)
    else:
        assert b"no HIP device" in lib.odef_last_error(None)
    assert lib.odef_create(C.byref(h), C.byref(_cfg(host, rhs_id=8))) != 0
    assert b"unknown rhs_id 8" in lib.odef_last_error(None)
    assert lib.odef_create(C.byref(h), C.byref(_cfg(host, d=3))) != 0
    assert b"dimension" in lib.odef_last_error(None)


def test_forced_kernels_in_the_code_object(pkg):
    """The lane kernels (both store variants, final-state mode, adaptive, MV, IEKS) and the row-team kernels of RhsForced."""
    pkg.load_library()
    obj = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build", "inst_forced.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    syms = [s for s in _kernel_symbols(obj) if "RhsForced" in s]
    for q in range(1, 6):
        for kernel in ("ek_filter_fixed_kernel", "ek_filter_adaptive_kernel", "ek_filter_fixed_mv_kernel", "ek_filter_adaptive_mv_kernel",
                       "ek_filter_fixed_ieks_kernel", "ek_filter_rows_kernel", "ek_filter_rows_adaptive_kernel", "ek_filter_rows_ieks_kernel"):
            assert any(kernel in s and f"RhsForcedELi{q}E" in s for s in syms), (kernel, q)
    for flags in ("Lb1ELb1ELb1E", "Lb1ELb1ELb0E", "Lb1ELb0ELb0E"):  # EK1: lagged stores, plain stores, final state
        assert any("ek_filter_fixed_kernel" in s and f"RhsForcedELi3E{flags}" in s for s in syms), flags


@pytest.mark.parametrize("with_jac", [True, False])
def test_has_time_struct_cross_compiles(pkg, with_jac):
    name = "TimeCabi" + ("Jac" if with_jac else "Fwd")
    pkg.compile_rhs(name, "struct " + name + " {" + FORCED_F + (FORCED_JAC if with_jac else "") + "};", 2, 3)


def test_has_time_with_the_three_argument_f_is_a_compile_error(pkg):
    src = """struct TimeCabiBad {
  static constexpr int d = 1, np = 1;
  static constexpr bool has_time = true;
  template <class T>
  __device__ static void f(const T (&u)[1], const double* p, T (&du)[1]) { du[0] = p[0] * u[0]; }
};"""
    with pytest.raises(pkg.OdefError, match="hipcc: compilation of the user vector field failed") as e:
        pkg.compile_rhs("TimeCabiBad", src, 1, 1)
    assert "error:" in str(e.value) and "rhs.h" in str(e.value)  # the compiler log


def test_has_time_field_of_team_size_is_refused(pkg):
    """d = 12, q = 2 would need the workgroup-per-trajectory kernels, which carry no time: odef_create says so, before any device
    is touched.  The same struct without has_time passes that check."""
    from odefilters_jl_amd import host

    body = """
  static constexpr int d = 12, np = 1;
  %s
  template <class T>
  __device__ static void f(const T (&u)[12], const double* p, %s T (&du)[12]) {
    for (int i = 0; i < 12; ++i) du[i] = p[0] * u[(i + 1) %% 12] %s;
  }
"""
    pkg.compile_rhs("TimeCabiBig", "struct TimeCabiBig {" + body % ("static constexpr bool has_time = true;", "T t,", "+ t") + "};", 12, 1)
    pkg.compile_rhs("TimeCabiBigAuto", "struct TimeCabiBigAuto {" + body % ("", "", "") + "};", 12, 1)
    lib = pkg.load_library()
    h = C.c_void_p()
    assert lib.odef_create(C.byref(h), C.byref(_cfg(host, rhs_id=host.RHS["TimeCabiBig"], d=12, n_params=1, order=2, alg=0))) != 0
    assert b"time-dependent fields run on the lane and row-team kernels" in lib.odef_last_error(None)
    import torch

    if not torch.cuda.is_available():  # (with a device this would go on to build the matrix-core module: minutes)
        assert lib.odef_create(C.byref(h), C.byref(_cfg(host, rhs_id=host.RHS["TimeCabiBigAuto"], d=12, n_params=1, order=2, alg=0))) != 0
        assert b"no HIP device" in lib.odef_last_error(None)
