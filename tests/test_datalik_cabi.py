"""Data log-likelihood without a GPU: the new ids in the header, the host layer and the Julia binding; no new entry point; what is
refused before a device is touched; the host layer's validation of times, components, data and noise; and the 19 kernels in the
gfx950 code object of their translation unit."""
import ctypes as C
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
NAMES = ["ODEF_L_BASE", "ODEF_L_DATA_LOGLIK", "ODEF_L_DATA_MAHALANOBIS", "ODEF_L_OBS_SAVE", "ODEF_L_OBS_COMPONENT", "ODEF_L_OBS_VALUE",
         "ODEF_L_OBS_NOISE"]
PAIRS = [(d, q) for d in range(1, 5) for q in range(1, 6) if d * (q + 1) <= 20]


def test_data_ids_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 1))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {", "  odef_data_field f = ODEF_L_OBS_NOISE;",
                     "  (void)f;", f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "datalik.c", tmp_path / "datalik"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, vals = vals[-1], dict(zip(NAMES, vals[:-1]))
    assert count == 18                                          # no new odef_field id
    assert vals == host.DATA_FIELDS
    assert vals == {"ODEF_L_BASE": 192, "ODEF_L_DATA_LOGLIK": 192, "ODEF_L_DATA_MAHALANOBIS": 193, "ODEF_L_OBS_SAVE": 200,
                    "ODEF_L_OBS_COMPONENT": 201, "ODEF_L_OBS_VALUE": 202, "ODEF_L_OBS_NOISE": 203}
    taken = set(range(0, 18)) | set(range(64, 84)) | set(range(128, 145))
    assert not taken & set(vals.values())
    assert not any(host._is_summary_field(v) or host._is_errors_field(v) for v in vals.values())
    assert (host.L_DATA_LOGLIK, host.L_DATA_MAHALANOBIS, host.L_OBS_SAVE, host.L_OBS_COMPONENT, host.L_OBS_VALUE,
            host.L_OBS_NOISE) == (192, 193, 200, 201, 202, 203)
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "function data_loglik" in jl
    assert len(host.SYMBOLS) == 44  # no new entry point


def test_calls_fail_loudly_before_a_device_is_touched(pkg):
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    b = C.c_size_t(7)
    buf = np.zeros(4)
    p = C.c_void_p()
    for f in host.DATA_FIELDS.values():
        assert lib.odef_field_bytes(None, f, C.byref(b)) == -1 and b.value == 7
        assert lib.odef_get(None, f, buf.ctypes.data_as(C.c_void_p), 32) == -1
        assert lib.odef_get_device(None, f, C.byref(p), C.byref(b)) == -1
        assert lib.odef_bind_device(None, f, None, 0) == -1
    assert hasattr(pkg.Context, "bind_observations") and hasattr(pkg.Context, "data_loglik")
    assert hasattr(host.DeviceGroup, "data_loglik") and hasattr(pkg.EnsembleSolution, "data_loglik")


def test_host_validation_of_the_observations(pkg):
    from odefilters_jl_amd import host

    t = np.arange(9) * 0.125
    s, c, v, r, per = host._observation_arrays(t, 3, 5, [0.25, 1.0], np.zeros((2, 2)), 0.5, (0, 2))
    assert list(s) == [2, 8] and s.dtype == np.int64 and list(c) == [0, 2] and v.shape == (2, 2) and list(r) == [0.5, 0.5] and not per
    s, c, v, r, per = host._observation_arrays(t, 3, 5, [0.0], np.arange(15.0).reshape(5, 1, 3), (1.0, 2.0, 3.0), None)
    assert list(s) == [0] and list(c) == [0, 1, 2] and per and v.shape == (1, 3, 5) and v[0, 1, 4] == 13.0   # [M][o][N]
    for kw, msg in ((dict(times=[0.25, 0.3]), "exactly"), (dict(times=[2.0]), "exactly"), (dict(times=[0.5, 0.25]), "increasing"),
                    (dict(components=(2, 0)), "components"), (dict(components=(0, 3)), "components"),
                    (dict(data=np.zeros((3, 2))), "shape"), (dict(noise_var=0.0), "positive"), (dict(noise_var=(1.0, np.inf)), "positive"),
                    (dict(noise_var=(1.0, 2.0, 3.0)), "noise_var")):
        a = dict(times=[0.25, 1.0], data=np.zeros((2, 2)), noise_var=0.5, components=(0, 2))
        a.update(kw)
        with pytest.raises(pkg.OdefError, match=msg):
            host._observation_arrays(t, 3, 5, a["times"], a["data"], a["noise_var"], a["components"])


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


def test_the_19_kernels_in_the_code_object(pkg):
    """datalik.o: data_loglik_kernel<d, q> for d <= 4, q <= 5, d (q + 1) <= 20 and nothing else out of line; no vector field's
    translation unit carries one.  A missing object or ROCm binutils is a failure, not a skip."""
    pkg.load_library()
    build = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build")
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    obj = os.path.join(build, "datalik.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    syms = sorted(set(_kernel_symbols(obj)))
    assert all("data_loglik_kernel" in s for s in syms), syms  # no device function out of line
    assert len(PAIRS) == 19 and len(syms) == 19, syms
    for d, q in PAIRS:
        assert any(f"data_loglik_kernelILi{d}ELi{q}E" in s for s in syms), (d, q, syms)
    assert not any("data_loglik" in s for s in _kernel_symbols(os.path.join(build, "inst_lorenz63.o")))
