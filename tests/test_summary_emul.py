"""Host build of the ensemble-summary reduction (tests/emul/emul_summary.cpp: csrc/summary_kernels.h, one thread per lane) against
the extended-precision reference, with the tolerances of the GPU tests: every trajectories-per-lane variant K, every d-mapping
(d = 2, 3, 10, 16, 28), ragged last workgroups, one trajectory, and trajectories dropped by their retcode, by an Inf and by a NaN.
ODEF_EMUL_SANITIZE=1 builds the library with AddressSanitizer + UBSan (tools/sanitize_emul.sh)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _summary_reference as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        san = os.environ.get("ODEF_EMUL_SANITIZE") == "1"
        src = os.path.join(HERE, "emul", "emul_summary.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_summary_san.so" if san else "libodef_emul_summary.so")
        deps = [src] + glob.glob(os.path.join(ROOT, "odefilters.jl_amd", "csrc", "summary*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else []
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-pthread", "-Wno-unknown-pragmas"] + flags + [src, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


CASES = [  # d, q, N, n_t, K
    (3, 3, 1, 2, 1), (3, 3, 63, 2, 8), (3, 3, 64, 1, 1), (3, 3, 65, 2, 2), (3, 3, 1001, 2, 4), (3, 3, 2500, 1, 8),
    (2, 1, 300, 2, 1), (10, 1, 700, 1, 2), (16, 2, 70, 1, 2), (28, 2, 5, 1, 1), (28, 1, 300, 1, 1),
]


@pytest.mark.parametrize("d,q,N,n_t,K", CASES, ids=[f"d{c[0]}-N{c[2]}-K{c[4]}" for c in CASES])
def test_emulated_reduction_against_the_reference(d, q, N, n_t, K):
    rng = np.random.default_rng(1000 * d + N)
    D = d * (q + 1)
    TRI, tri = D * (D + 1) // 2, d * (d + 1) // 2
    mean = rng.uniform(-27, 27, (n_t, D, 1)) + 10.0 ** rng.uniform(-6, -2, (n_t, 1, 1)) * rng.standard_normal((n_t, D, N))
    cov = np.ascontiguousarray(rng.uniform(-1e-6, 1e-6, (n_t, TRI, N)))
    rc = np.zeros(N, np.int32)
    dropped = 0
    if N > 10:
        rc[7] = 3
        mean[0, d - 1, 3] = np.inf
        mean[0, 0, N - 1] = np.nan
        dropped = 3
    mean = np.ascontiguousarray(mean)
    cnt, m, w, b = np.zeros(n_t, np.int64), np.zeros((n_t, d)), np.zeros((n_t, tri)), np.zeros((n_t, tri))
    assert lib().emul_summary(K, _p(mean), _p(cov), _p(rc, C.c_int), C.c_long(N), C.c_long(n_t), d, D, TRI, _p(cnt, C.c_longlong),
                              _p(m), _p(w), _p(b)) == 0
    ref = sr.reference(mean, cov, rc, d)
    assert ref[0][0] == N - dropped
    worst = sr.check((cnt, m, w, b), ref, d, label=f"d={d} N={N} K={K}")
    print(f"d={d} N={N} K={K}: error / bound  MEAN {worst[0]:.3g}  COV_WITHIN {worst[1]:.3g}  COV_BETWEEN {worst[2]:.3g}")


def test_no_trajectory_included_gives_nan():
    d, D, N = 3, 6, 70
    mean, cov, rc = np.ones((1, D, N)), np.ones((1, D * (D + 1) // 2, N)), np.ones(N, np.int32)
    cnt, m, w, b = np.zeros(1, np.int64), np.zeros((1, d)), np.zeros((1, 6)), np.zeros((1, 6))
    assert lib().emul_summary(2, _p(mean), _p(cov), _p(rc, C.c_int), C.c_long(N), C.c_long(1), d, D, D * (D + 1) // 2,
                              _p(cnt, C.c_longlong), _p(m), _p(w), _p(b)) == 0
    assert cnt[0] == 0 and np.all(np.isnan(m)) and np.all(np.isnan(w)) and np.all(np.isnan(b))
