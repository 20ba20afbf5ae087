"""Data log-likelihood at arbitrary times without a GPU: the new id in the header, the host layer and the Julia binding; no new
entry point; what is refused before a device is touched; the host layer's choice between the save path and the time path and its
validation of the times; and the 15 kernels in the gfx950 code object of their translation unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_datalik_cabi import LLVM, ROOT, _kernel_symbols

PAIRS = [(d, q) for d in range(1, 5) for q in range(1, 6) if d * (q + 1) <= 12]


def test_the_time_id_in_header_host_and_julia(pkg, tmp_path):
    from odefilters_jl_amd import host

    src = "\n".join(['#include <stdio.h>', '#include "odefilter.h"', "int main(void) {", "  odef_data_field f = ODEF_L_OBS_TIME;",
                     '  printf("%d %d %d\\n", (int)f, (int)ODEF_L_OBS_NOISE, (int)ODEF_F_COUNT_);', "  return 0;", "}"])
    cfile, exe = tmp_path / "dlt.c", tmp_path / "dlt"
    cfile.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    t, noise, count = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (t, noise, count) == (204, 203, 18)                  # the id follows the other inputs; no new odef_field id
    assert host.L_OBS_TIME == 204 and host.DATA_TIME_FIELDS == {"ODEF_L_OBS_TIME": 204}
    assert not (host._is_summary_field(204) or host._is_errors_field(204) or host._is_event_field(204)) and 204 not in host._DERIVED
    jl = open(os.path.join(ROOT, "julia", "ODEFilterHIP.jl")).read()
    m = re.search(r"\bL_OBS_TIME = (\d+)", jl)
    assert m and int(m.group(1)) == 204 and "function data_loglik_times" in jl
    assert len(host.SYMBOLS) == 44                              # no new entry point


def test_calls_fail_loudly_before_a_device_is_touched(pkg):
    from odefilters_jl_amd import host

    lib = pkg.load_library()
    b = C.c_size_t(7)
    p = C.c_void_p()
    assert lib.odef_field_bytes(None, 204, C.byref(b)) == -1 and b.value == 7
    assert lib.odef_get_device(None, 204, C.byref(p), C.byref(b)) == -1
    assert lib.odef_bind_device(None, 204, None, 0) == -1
    assert hasattr(pkg.Context, "bind_observation_times")


def test_host_choice_of_the_path_and_validation_of_the_times(pkg):
    from odefilters_jl_amd import host

    t = np.arange(9) * 0.125
    assert host._on_grid(t, [0.25, 1.0]) and host._on_grid(t, [0.0]) and host._on_grid(t, [0.5, 0.25])
    assert not host._on_grid(t, [0.25, 0.3]) and not host._on_grid(t, [np.nextafter(0.25, 1.0)]) and not host._on_grid(t, [2.0])
    tm, c, v, r, per = host._observation_time_arrays(3, 5, [0.1, 0.25, 0.26], np.zeros((3, 2)), 0.5, (0, 2), t[0], t[-1])
    assert tm.dtype == np.float64 and list(tm) == [0.1, 0.25, 0.26] and list(c) == [0, 2] and v.shape == (3, 2) and not per
    tm, c, v, r, per = host._observation_time_arrays(3, 5, [0.3], np.arange(15.0).reshape(5, 1, 3), (1.0, 2.0, 3.0), None)
    assert per and v.shape == (1, 3, 5) and v[0, 1, 4] == 13.0 and list(c) == [0, 1, 2]
    for kw, msg in ((dict(times=[0.3, 0.3]), "increasing"), (dict(times=[0.5, 0.25]), "increasing"), (dict(times=[0.1, np.inf]), "finite"),
                    (dict(times=[np.nan]), "finite"), (dict(times=[-0.1, 0.2]), "before the first save"),
                    (dict(times=[0.1, 1.0 + 1e-9]), "above the last save"), (dict(times=[]), "non-empty"),
                    (dict(components=(2, 0)), "components"), (dict(data=np.zeros((3, 2))), "shape"), (dict(noise_var=0.0), "positive")):
        a = dict(times=[0.25, 0.9], data=np.zeros((2, 2)), noise_var=0.5, components=(0, 2))
        a.update(kw)
        with pytest.raises(pkg.OdefError, match=msg):
            host._observation_time_arrays(3, 5, a["times"], a["data"], a["noise_var"], a["components"], t[0], t[-1])
    # an adaptive solve has no shared last save: a late time is left to the device (NaN for the trajectories that end before it)
    host._observation_time_arrays(3, 5, [0.1, 7.0], np.zeros((2, 2)), 0.5, (0, 2), 0.0, None)


def test_the_15_kernels_in_the_code_object(pkg):
    """datalik_times.o: data_loglik_times_kernel<d, q> for d <= 4, q <= 5, d (q + 1) <= 12 and nothing else out of line; the
    translation unit of the save path and a vector field's carry none.  A missing object or ROCm binutils is a failure, not a skip."""
    pkg.load_library()
    build = os.path.join(ROOT, "odefilters.jl_amd", "csrc", "build")
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "ROCm binutils missing"
    obj = os.path.join(build, "datalik_times.o")
    assert os.path.exists(obj), f"{obj} missing: build the library first"
    syms = sorted(set(_kernel_symbols(obj)))
    assert all("data_loglik_times_kernel" in s for s in syms), syms  # no device function out of line
    assert len(PAIRS) == 15 and len(syms) == 15, syms
    for d, q in PAIRS:
        assert any(f"data_loglik_times_kernelILi{d}ELi{q}E" in s for s in syms), (d, q, syms)
    for other in ("datalik.o", "inst_lorenz63.o"):
        assert not any("data_loglik_times" in s for s in _kernel_symbols(os.path.join(build, other)))
