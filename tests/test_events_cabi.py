"""Event location without a GPU: the new ids in the header, the host layer and the Julia binding; no new entry point and no new
odef_field id; what is refused before a device is touched; the host layer's validation of component, direction, K and level; and the
16 kernels in the gfx950 code object of their translation unit."""
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
QUANTITIES = ["COUNT", "TIME", "TIME_VAR", "U", "DIRECTION", "SAVE", "NEVAL"]
NAMES = (["ODEF_EV_BASE"] + [f"ODEF_EV_{q}" for q in QUANTITIES] + [f"ODEF_EV_SMOOTH_{q}" for q in QUANTITIES] +
         ["ODEF_EV_SPEC", "ODEF_EV_LEVEL"])
PAIRS = [(d, q) for d in range(1, 5) for q in range(1, 6) if d * (q + 1) <= 12]


def test_event_ids_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    fmt = " ".join(["%d"] * (len(NAMES) + 1))
    args = ", ".join(f"(int){n}" for n in NAMES + ["ODEF_F_COUNT_"])
    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {", "  odef_event_field f = ODEF_EV_LEVEL;",
                     "  (void)f;", f'  printf("{fmt}\\n", {args});', "  return 0;", "}"])
    cfile, exe = tmp_path / "events.c", tmp_path / "events"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    count, vals = vals[-1], dict(zip(NAMES, vals[:-1]))
    assert count == 18                                          # no new odef_field id
    assert vals == host.EVENT_FIELDS
    assert vals["ODEF_EV_BASE"] == 256 and vals["ODEF_EV_SPEC"] == 280 and vals["ODEF_EV_LEVEL"] == 281
    for s, prefix in enumerate(("ODEF_EV_", "ODEF_EV_SMOOTH_")):
        for k, q in enumerate(QUANTITIES):
            assert vals[prefix + q] == 256 + 8 * s + k == host.event_field(s, k)
            assert host._is_event_field(vals[prefix + q])
    taken = set(range(0, 18)) | set(range(64, 84)) | set(range(128, 145)) | set(range(192, 204))
    assert not taken & set(vals.values())
    assert not any(host._is_summary_field(v) or host._is_errors_field(v) for v in vals.values())
    assert not host._is_event_field(280) and not host._is_event_field(263) and not host._is_event_field(272)
    assert (host.EV_BASE, host.EV_SPEC, host.EV_LEVEL, host.K_EVENTS) == (256, 280, 281, 5)
    with pytest.raises(pkg.OdefError):
        host.event_field(2, 0)
    with pytest.raises(pkg.OdefError):
        host.event_field(0, 7)
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    for k, v in vals.items():
        m = re.search(rf"\b{k[5:]} = (\d+)", jl)  # the Julia constants drop the ODEF_ prefix
        assert m and int(m.group(1)) == v, k
    assert "function events" in jl
    assert len(host.SYMBOLS) == 44  # no new entry point


def test_calls_fail_loudly_before_a_device_is_touched(pkg):
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    b = C.c_size_t(7)
    buf = np.zeros(4)
    p = C.c_void_p()
    for f in host.EVENT_FIELDS.values():
        assert lib.odef_field_bytes(None, f, C.byref(b)) == -1 and b.value == 7
        assert lib.odef_get(None, f, buf.ctypes.data_as(C.c_void_p), 32) == -1
        assert lib.odef_get_device(None, f, C.byref(p), C.byref(b)) == -1
        assert lib.odef_bind_device(None, f, None, 0) == -1
    ms, n = C.c_float(), C.c_int()
    assert lib.odef_kernel_time_ms(None, 5, C.byref(ms), C.byref(n)) == -1
    assert hasattr(pkg.Context, "bind_event") and hasattr(pkg.Context, "events")
    assert hasattr(host.DeviceGroup, "events") and hasattr(pkg.EnsembleSolution, "events") and hasattr(pkg, "Events")


def test_host_validation_of_the_spec(pkg):
    from odefilters_jl_amd import host

    spec, lvl = host._event_arrays(3, 5, 2, 0.25, -1, 4)
    assert spec.dtype == np.int64 and list(spec) == [2, -1, 4] and lvl.dtype == np.float64 and list(lvl) == [0.25]
    spec, lvl = host._event_arrays(3, 5, 0, np.arange(5.0), 0, 1)
    assert list(spec) == [0, 0, 1] and lvl.shape == (5,) and lvl.flags.c_contiguous
    for kw, msg in ((dict(component=3), "component"), (dict(component=-1), "component"), (dict(component=0.5), "component"),
                    (dict(direction=2), "direction"), (dict(max_events=0), "max_events"), (dict(max_events=1.5), "max_events"),
                    (dict(level=np.zeros(4)), "level"), (dict(level=np.zeros((5, 1))), "level")):
        a = dict(component=1, level=0.0, direction=0, max_events=2)
        a.update(kw)
        with pytest.raises(pkg.OdefError, match=msg):
            host._event_arrays(3, 5, a["component"], a["level"], a["direction"], a["max_events"])


def test_the_events_dataclass_is_trajectory_major(pkg):
    K, d, N = 2, 3, 4
    abi = [np.arange(N, dtype=np.int32), np.arange(K * N, dtype=float).reshape(K, N), np.full((K, N), 4.0),
           np.arange(K * d * N, dtype=float).reshape(K, d, N), np.ones((K, N), np.int32), np.zeros((K, N), np.int32),
           np.full((K, N), 3, np.int32)]
    abi[2][1, 2] = np.nan
    e = pkg.Events.from_abi(abi)
    assert e.count.shape == (N,) and e.t.shape == (N, K) and e.u.shape == (N, K, d) and e.save.shape == (N, K)
    assert e.t[3, 1] == abi[1][1, 3] and e.u[2, 1, 0] == abi[3][1, 0, 2] and e.t_std[0, 0] == 2.0 and np.isnan(e.t_std[2, 1])
    both = pkg.Events.concatenate([e, e])
    assert both.count.shape == (2 * N,) and both.u.shape == (2 * N, K, d) and np.array_equal(both.t[N:], e.t)


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


def test_both_kernels_in_the_code_object_and_no_device_function(pkg):
    """events.o: event_scan_kernel, event_refine_kernel<d, q> for d <= 4, q <= 5, d (q + 1) <= 12 and nothing else out of line; no
    vector field's translation unit carries one.  A missing object or ROCm binutils is a failure, not a skip."""
    pkg.load_library()
    build = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build")
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    obj = os.path.join(build, "events.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    syms = sorted(set(_kernel_symbols(obj)))
    assert all("event_scan_kernel" in s or "event_refine_kernel" in s for s in syms), syms  # no device function out of line
    assert len(PAIRS) == 15 and len(syms) == 16, syms
    assert sum("event_scan_kernel" in s for s in syms) == 1
    for d, q in PAIRS:
        assert any(f"event_refine_kernelILi{d}ELi{q}E" in s for s in syms), (d, q, syms)
    assert not any("event_" in s for s in _kernel_symbols(os.path.join(build, "inst_lorenz63.o")))
