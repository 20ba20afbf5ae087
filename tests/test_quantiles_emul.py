"""Host build of the ensemble-quantile kernels (tests/emul/emul_quantiles.cpp: csrc/quantile_kernels.h, one thread per lane of a
workgroup, the launch sequence of quantiles.hip) against tests/_quantile_reference.py, exactly: every N at which the mapping
changes (1, 2, one lane short of / exactly / one past a wavefront, more than a workgroup, ragged chunks, more than one chunk per
row, more than one slab), every d-mapping (2, 3, 16, 28), P = 1, 3, 8 with unsorted and repeated probabilities, rows that break a
wrong key transform or tie rule, and trajectories dropped by their retcode, by an Inf in another component and by a NaN at one
time.  The same source with its own main() is built with AddressSanitizer + UBSan and run as a stand-alone program."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _quantile_reference as qr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emul", "emul_quantiles.cpp")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(HERE, "emul", "libodef_emul_quantiles.so")
        deps = [SRC] + glob.glob(os.path.join(ROOT, "odefilters.jl_amd", "csrc", "quantile*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                                   "-Wno-unknown-pragmas", SRC, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def emulate(mean, rc, d, probs, iters, slab):
    mean = np.ascontiguousarray(mean, np.float64)
    rc = np.ascontiguousarray(rc, np.int32)
    probs = np.ascontiguousarray(probs, np.float64)
    n_t, D, N = mean.shape
    cnt, q = np.full(n_t, -7, np.int64), np.full((n_t, probs.size, d), 123.0)
    passes = C.c_int(-1)
    assert lib().emul_quantiles(_p(mean), _p(rc, C.c_int), C.c_long(N), C.c_long(n_t), d, D, probs.size, _p(probs), iters,
                                C.c_long(slab), _p(cnt, C.c_longlong), _p(q), C.byref(passes)) == 0
    return (cnt, q), passes.value


def row_values(kind, N, rng):
    """One row of N values of a kind that breaks a wrong key transform or a wrong tie rule."""
    if kind == 0:  # mixed signs
        return rng.standard_normal(N)
    if kind == 1:  # +0 and -0 among small values of both signs
        return rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3]), N)
    if kind == 2:  # denormals of both signs, and zero
        return rng.integers(-50, 50, N).astype(np.float64) * 4.9406564584124654e-324
    if kind == 3:  # magnitudes from 1e-300 to 1e300 in one row, both signs
        return rng.choice(np.array([-1.0, 1.0]), N) * 10.0 ** rng.uniform(-300, 300, N)
    if kind == 4:  # all equal
        return np.full(N, -2.718281828)
    if kind == 5:  # 90 % duplicates
        return np.where(rng.uniform(size=N) < 0.9, 1.5, rng.uniform(1.0, 2.0, N))
    if kind == 6:  # values that differ only in the last mantissa bit
        return np.where(rng.integers(0, 2, N) == 1, np.nextafter(27.0, 28.0), 27.0)
    return 27.0 + 1e-6 * rng.standard_normal(N)  # a realistic row


def make_records(N, n_t, d, D, seed, drop=True):
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((n_t, D, N))
    for s in range(n_t):
        for a in range(d):
            mean[s, a] = row_values((s * d + a) % 8, N, rng)
    rc = np.zeros(N, np.int32)
    if drop and N > 10:
        rc[7] = 3                        # by retcode
        mean[0, d - 1, 3] = np.inf       # by an Inf in another component
        mean[n_t - 1, 0, N - 1] = np.nan  # by a NaN at one time only
    return mean, rc


P8 = qr.PROBS8
P8_REPEATED = np.array([0.95, 0.0, 0.5, 1.0 / 3.0, 0.05, 1.0, 0.5, 0.75])
P3 = np.array([0.95, 0.05, 0.5])
P1 = np.array([1.0 / 3.0])

CASES = [  # N, n_t, d, D, probs, iters, slab
    (1, 4, 2, 4, P1, 1, 4), (2, 3, 3, 6, P3, 1, 2), (63, 4, 2, 2, P8, 1, 3), (64, 3, 3, 12, P3, 2, 1),
    (65, 1, 16, 32, P3, 1, 1), (257, 1, 28, 28, P1, 1, 1), (257, 3, 3, 6, P8_REPEATED, 1, 3), (1001, 3, 3, 6, P8, 2, 2),
    (2500, 3, 3, 3, P3, 4, 2),
]


@pytest.mark.parametrize("N,n_t,d,D,probs,iters,slab", CASES, ids=[f"N{c[0]}-d{c[2]}-P{c[4].size}" for c in CASES])
def test_emulated_selection_equals_the_reference(N, n_t, d, D, probs, iters, slab):
    mean, rc = make_records(N, n_t, d, D, seed=100 * d + N)
    got, passes = emulate(mean, rc, d, probs, iters, slab)
    want = qr.reference(mean, rc, d, probs)
    if N > 10:
        assert want[0][0] == want[0][-1] == (N - 2 if n_t > 1 else N - 3)
    qr.check(got, want, label=f"N={N} d={d}")
    assert passes == qr.expected_passes(mean, rc, d, slab)  # the offset keys' width decides, slab by slab


def test_every_trajectory_dropped_gives_nan_and_count_zero():
    mean, rc = make_records(70, 2, 2, 4, seed=5, drop=False)
    rc[:] = 2
    (cnt, q), passes = emulate(mean, rc, 2, P3, 1, 2)
    assert cnt.tolist() == [0, 0] and np.all(np.isnan(q)) and passes == 0
    rc[:] = 0
    mean[1, 1, :] = np.nan  # every trajectory dropped at one time only
    got, _ = emulate(mean, rc, 2, P3, 1, 1)
    want = qr.reference(mean, rc, 2, P3)
    assert want[0].tolist() == [70, 0]
    qr.check(got, want, label="one empty time")


def test_the_shared_prefix_saves_digit_passes():
    """A row of value 27 with a spread of 1e-6 is 2e-6 / ulp(27) = 2^29.1 keys wide: 30 bits, four of the eight passes -- although
    the row straddles 27.0, where the keys themselves share 15 leading bits only.  Rows that are all equal need no pass."""
    rng = np.random.default_rng(11)
    mean = (27.0 + 1e-6 * rng.uniform(-1, 1, (1, 2, 300)))
    got, passes = emulate(mean, np.zeros(300, np.int32), 2, P3, 1, 1)
    qr.check(got, qr.reference(mean, np.zeros(300, np.int32), 2, P3), label="realistic")
    assert passes == 4 == qr.expected_passes(mean, np.zeros(300, np.int32), 2, 1)
    k = qr.keys(mean[0, 0])
    assert int(k.min() ^ k.max()).bit_length() > 48  # the keys themselves differ in a bit above 48: seven passes on raw prefixes
    mean[:] = 27.0
    got, passes = emulate(mean, np.zeros(300, np.int32), 2, P3, 1, 1)
    assert passes == 0 and np.all(got[1] == 27.0)


def test_stand_alone_program_is_clean_under_the_sanitizers(tmp_path):
    """The same source with -DODEF_EMUL_MAIN: its own main, AddressSanitizer + UBSan, run as a subprocess (no Python in it)."""
    exe = tmp_path / "emul_quantiles_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas", "-DODEF_EMUL_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("clean")
