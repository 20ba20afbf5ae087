"""Solution errors without a GPU: the new ids in the header, the host layer and the Julia binding; what is refused before a device
is touched; the error kernels in the gfx950 code objects of their translation units; and `odef_rhs_compile` of user vector fields
with and without an `analytic` member (a hipcc child process, no GPU)."""
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
QUANTITIES = ("FINAL", "L2", "LINF", "CHI2", "NUSED", "U_ANALYTIC")
NAMES = ["ODEF_E_BASE"] + [f"ODEF_E_{q}" for q in QUANTITIES] + [f"ODEF_E_SMOOTH_{q}" for q in QUANTITIES] + ["ODEF_E_REFERENCE"]


def test_error_ids_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 2))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_", "ODEF_S_DENSE_COV_BETWEEN"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {",
                     "  odef_errors_field f = ODEF_E_SMOOTH_U_ANALYTIC;", "  (void)f;",
                     f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "errors.c", tmp_path / "errors"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, last_summary, vals = vals[-2], vals[-1], dict(zip(NAMES, vals[:-2]))
    assert count == 18                                          # no new odef_field id
    assert all(v > last_summary for v in vals.values())         # clear of the summary's 64 + 8 source + quantity range
    ids = [v for k, v in vals.items() if k != "ODEF_E_BASE"]
    assert len(set(ids)) == len(ids) == 13
    assert vals == host.ERRORS_FIELDS
    for s, prefix in enumerate(("ODEF_E_", "ODEF_E_SMOOTH_")):
        for q, name in enumerate(QUANTITIES):
            assert host.errors_field(s, q) == vals[prefix + name] == vals["ODEF_E_BASE"] + 8 * s + q
    assert host.E_REFERENCE == vals["ODEF_E_REFERENCE"] and not host._is_errors_field(host.E_REFERENCE)
    assert all(host._is_errors_field(v) for k, v in vals.items() if k != "ODEF_E_REFERENCE")
    assert not any(host._is_summary_field(v) for v in vals.values())
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "solution_errors" in jl
    assert len(host.SYMBOLS) == 44  # no new entry point


def test_refusals_before_a_device_is_touched(pkg):
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    b = C.c_size_t(7)
    for f in (host.errors_field(0, host.E_L2), host.errors_field(1, host.E_U_ANALYTIC), host.E_REFERENCE):
        assert lib.odef_field_bytes(None, f, C.byref(b)) == -1 and b.value == 7
    assert lib.odef_bind_device(None, host.E_REFERENCE, None, 0) == -1
    for source, qty in ((2, 0), (-1, 0), (0, 6), (1, -1)):
        with pytest.raises(pkg.OdefError, match="no solution-error field"):
            host.errors_field(source, qty)
    assert hasattr(pkg.Context, "solution_errors") and hasattr(pkg.Context, "bind_reference")
    assert hasattr(host.DeviceGroup, "solution_errors")
    assert isinstance(pkg.EnsembleSolution.errors, property) and isinstance(pkg.EnsembleSolution.u_analytic, property)


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


def test_error_kernels_in_the_code_objects(pkg):
    """errors.o: errors_partial_kernel<DR, TruthBuffer> for DR = 0 (LDS column) and 1..8 (registers) and the fold kernel, nothing
    else out of line.  inst_linear.o: the partial and the truth kernel around RhsLinear's analytic.  A missing object or ROCm
    binutils is a failure, not a skip."""
    pkg.load_library()
    build = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build")
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    obj = os.path.join(build, "errors.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    syms = _kernel_symbols(obj)
    for dr in range(9):
        assert any("errors_partial_kernel" in s and f"ILi{dr}E" in s and "TruthBuffer" in s for s in syms), (dr, syms)
    assert any("errors_fold_kernel" in s for s in syms)
    assert all("kernel" in s for s in syms), syms
    lin = _kernel_symbols(os.path.join(build, "inst_linear.o"))
    assert any("errors_partial_kernel" in s and "ILi2E" in s and "TruthAnalytic" in s and "RhsLinear" in s for s in lin), lin
    assert any("errors_truth_kernel" in s and "RhsLinear" in s for s in lin), lin
    assert not any("errors_" in s for s in _kernel_symbols(os.path.join(build, "inst_lorenz63.o")))  # a field without analytic


USER_DECAY = """
struct NAME {
  static constexpr int d = 1, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[1], const double* p, T (&du)[1]) { du[0] = -p[0] * u[0]; }
ANALYTIC
};
"""
GOOD = """  template <class T>
  __device__ static void analytic(const T (&u0)[1], const double* p, T t, T (&out)[1]) { out[0] = u0[0] * exp(-p[0] * t); }"""
# (a template: nothing looks into its body until the error kernels instantiate it)
BAD = """  template <class T>
  __device__ static void analytic(const T (&u0)[1], const double* p, T t, T (&out)[1]) { out[0] = u0[0].no_such_member(t); }"""


def test_rhs_compile_with_and_without_analytic(pkg):
    """A user field may carry `analytic`: its error kernels are compiled with the field's module, so a body that does not compile
    is reported by odef_rhs_compile with the compiler's log; a field without one compiles as before."""
    from odefilters_jl_amd import host as h

    assert h.RHS[pkg.compile_rhs("DecayPlain", USER_DECAY.replace("NAME", "DecayPlain").replace("ANALYTIC", ""), 1, 1)] >= 100
    assert h.RHS[pkg.compile_rhs("DecayTruth", USER_DECAY.replace("NAME", "DecayTruth").replace("ANALYTIC", GOOD), 1, 1)] >= 100
    with pytest.raises(pkg.OdefError, match="no_such_member"):
        pkg.compile_rhs("DecayBroken", USER_DECAY.replace("NAME", "DecayBroken").replace("ANALYTIC", BAD), 1, 1)
