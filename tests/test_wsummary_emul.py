"""Host build of the weighted ensemble-summary kernels (tests/emul/emul_wsummary.cpp: csrc/wsummary_kernels.h, one thread per lane
of a wavefront, the launch sequence of wsummary.hip) against tests/_wsummary_reference.py within the derived bounds of DESIGN.md
3.19, with no factor on top: every N at which the mapping changes (1, 2, one lane short of / exactly / one past a wavefront, more
than a workgroup, ragged workgroups, several workgroups per time), d = 2, 3, 10, 16, 28 and every K, n_t = 1 and 5, and the
weight patterns -- all equal (against the UNWEIGHTED reference), a common offset of 1e6, a spread of 800 that underflows, one
dominant weight, NaN / +inf / -inf entries, trajectories dropped by retcode and by a NaN at one time, the carrier of the maximum
dropped at one time (Z == 0), a time with nobody, no finite weight at all.  Two runs agree bit for bit.  The same source with its
own main() is built with AddressSanitizer + UBSan and run as a stand-alone program."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _summary_reference as sr
import _wsummary_reference as wr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emul", "emul_wsummary.cpp")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(HERE, "emul", "libodef_emul_wsummary.so")
        deps = [SRC] + glob.glob(os.path.join(ROOT, "odefilters.jl_amd", "csrc", "wsummary*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                                   "-Wno-unknown-pragmas", SRC, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def emulate(mean, cov, rc, logw, d, K, max_blocks=1024):
    mean = np.ascontiguousarray(mean, np.float64)
    cov = np.ascontiguousarray(cov, np.float64)
    rc = np.ascontiguousarray(rc, np.int32)
    logw = np.ascontiguousarray(logw, np.float64)
    n_t, D, N = mean.shape
    TRI, T = cov.shape[1], wr.tri(d)
    cnt = np.full(n_t, -7, np.int64)
    m, w, b = np.full((n_t, d), 123.0), np.full((n_t, T), 123.0), np.full((n_t, T), 123.0)
    le, ess = np.full(n_t, 123.0), np.full(n_t, 123.0)
    assert lib().emul_wsummary(K, _p(mean), _p(cov), _p(rc, C.c_int), _p(logw), C.c_long(N), C.c_long(n_t), d, D, TRI, max_blocks,
                               _p(cnt, C.c_longlong), _p(m), _p(w), _p(b), _p(le), _p(ess)) == 0
    return cnt, m, w, b, le, ess


def make_records(N, n_t, d, D, seed, drop=True):
    """Means of order 10 with a spread of order 1 (a centred second moment that cancels), covariances of mixed sign off the
    diagonal; with `drop` one trajectory left out by its retcode and one by a NaN at the last time only."""
    rng = np.random.default_rng(seed)
    TRI = D * (D + 1) // 2
    mean = 10.0 + rng.standard_normal((n_t, D, N))
    cov = 1e-3 * rng.standard_normal((n_t, TRI, N))
    rc = np.zeros(N, np.int32)
    if drop and N > 10:
        rc[7] = 3
        mean[n_t - 1, d - 1, N - 1] = np.nan
    return mean, cov, rc


def realistic(N, rng):
    """Log-likelihoods of order -100 with a spread of tens, on a grid of 2^-20 so that adding 1e6 is exact."""
    return np.round((-100.0 - 20.0 * rng.standard_normal(N) ** 2) * 2.0 ** 20) / 2.0 ** 20


def run_and_check(label, mean, cov, rc, logw, d, K, values=None):
    got = emulate(mean, cov, rc, logw, d, K)
    ref = wr.reference(mean, cov, rc, logw, d)
    worst = wr.check(got, ref, d, label=label, values=values)  # (prints every ratio; DESIGN.md 3.19 quotes the worst)
    print(f"{label}: worst error / bound  " + "  ".join(f"{n} {r:.3g}" for n, r in zip(wr.NAMES, worst)))
    return got, ref


SHAPES = [  # N, n_t, d, D, K: every N of the mapping, every d, every K, n_t = 1 and 5
    (1, 1, 2, 4, 1), (2, 5, 3, 6, 8), (63, 5, 2, 2, 8), (64, 1, 3, 12, 4), (65, 5, 10, 20, 2), (257, 1, 28, 28, 1), (257, 1, 16, 32, 2),
    (1001, 5, 3, 6, 4), (1001, 1, 10, 10, 2), (2500, 5, 2, 4, 8), (2500, 1, 3, 3, 2),
]
# one shape per K for the weight patterns: ragged, more than one workgroup per time where K allows it at these sizes
BY_K = {1: (300, 2, 10, 10), 2: (700, 2, 10, 20), 4: (1100, 5, 3, 6), 8: (2500, 5, 2, 4)}


@pytest.mark.parametrize("N,n_t,d,D,K", SHAPES, ids=[f"N{c[0]}-d{c[2]}-K{c[4]}-t{c[1]}" for c in SHAPES])
def test_realistic_weights_on_every_mapping(N, n_t, d, D, K):
    mean, cov, rc = make_records(N, n_t, d, D, seed=100 * d + N)
    logw = realistic(N, np.random.default_rng(N + d))
    got, ref = run_and_check(f"realistic N={N} d={d} K={K}", mean, cov, rc, logw, d, K)
    if N > 10:
        assert ref["count"][0] == (N - 1 if n_t > 1 else N - 2) and ref["count"][-1] == N - 2
    again = emulate(mean, cov, rc, logw, d, K)
    for a, b in zip(got, again):  # the order of every sum is fixed: two runs agree bit for bit
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_equal_weights_meet_the_unweighted_reference(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=K)
    ell = 3.25
    logw = np.full(N, ell)
    cnt, m, w, b, _, _ = sr.reference(mean, cov, rc, d)
    ref = wr.reference(mean, cov, rc, logw, d)
    assert np.array_equal(cnt, ref["count"])
    unweighted = {"mean": m, "within": w, "between": b, "log_evidence": np.full(n_t, ell, np.longdouble),
                  "ess": cnt.astype(np.longdouble)}
    run_and_check(f"equal K={K}", mean, cov, rc, logw, d, K, values=unweighted)


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_a_common_offset_moves_the_log_evidence_only(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=10 + K)
    logw = realistic(N, np.random.default_rng(K))
    assert np.array_equal((logw + 1e6) - 1e6, logw)  # the offset is exact on this grid
    base, ref = run_and_check(f"realistic K={K}", mean, cov, rc, logw, d, K)
    off, _ = run_and_check(f"offset K={K}", mean, cov, rc, logw + 1e6, d, K)
    moved = dict(ref)
    moved["log_evidence"] = ref["log_evidence"] + np.longdouble(1e6)
    wr.check(off, ref, d, label=f"offset against the un-offset reference K={K}", values=moved)
    for k in (0, 1, 2, 3, 5):  # the shifted weights are the same doubles
        assert off[k].tobytes() == base[k].tobytes()


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_a_spread_of_800_underflows_and_still_counts(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=20 + K)
    logw = np.random.default_rng(K).permutation(np.linspace(0.0, -800.0, N))
    got, ref = run_and_check(f"spread K={K}", mean, cov, rc, logw, d, K)
    assert np.exp(-800.0) == 0.0 and ref["count"][0] == N - 1  # underflowed weights still count
    assert np.all(got[5] < 10.0) and np.all(got[5] >= 1.0)  # of hundreds to thousands included


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_one_dominant_weight(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=30 + K)
    logw = realistic(N, np.random.default_rng(K)) - 60.0
    logw[N // 2] = 0.0
    got, _ = run_and_check(f"dominant K={K}", mean, cov, rc, logw, d, K)
    np.testing.assert_allclose(got[1][0], mean[0, :d, N // 2], rtol=1e-12)
    assert np.all(got[5] < 1.0 + 1e-9)


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_weights_that_are_not_finite_exclude_their_trajectories(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=40 + K)
    logw = realistic(N, np.random.default_rng(K))
    logw[[3, 64, N - 2]] = np.nan, np.inf, -np.inf
    logw[7] = 1e9  # the largest of all belongs to a trajectory that did not succeed: it must not become L
    _, ref = run_and_check(f"non-finite K={K}", mean, cov, rc, logw, d, K)
    assert ref["count"][0] == N - 4 and ref["count"][-1] == N - 5  # retcode, three weights; and a NaN mean at the last time


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_the_carrier_of_the_maximum_dropped_at_one_time_and_a_time_with_nobody(K):
    N, n_t, d, D = BY_K[K]
    mean, cov, rc = make_records(N, n_t, d, D, seed=50 + K, drop=False)
    logw = -800.0 - (np.arange(N) % 7)  # exp underflows for every one of them
    logw[N // 3] = 0.0
    mean[0, 0, N // 3] = np.inf  # Z == 0 at time 0: NaN moments, NaN ESS, LOG_EVIDENCE -inf, COUNT N - 1
    mean[n_t - 1, d - 1, :] = np.nan  # nobody at the last time
    got, ref = run_and_check(f"Z == 0 K={K}", mean, cov, rc, logw, d, K)
    assert got[0][0] == N - 1 and got[4][0] == -np.inf and np.isnan(got[5][0]) and np.all(np.isnan(got[1][0]))
    assert got[0][-1] == 0 and np.isnan(got[4][-1]) and np.all(np.isnan(got[3][-1]))
    if n_t > 2:
        assert np.all(np.isfinite(got[1][1])) and abs(got[5][1] - 1.0) < 1e-12


def test_no_finite_weight_at_all():
    mean, cov, rc = make_records(70, 2, 2, 4, seed=5, drop=False)
    logw = np.where(np.arange(70) % 2 == 0, np.nan, -np.inf)
    got = emulate(mean, cov, rc, logw, 2, 1)
    assert got[0].tolist() == [0, 0]
    assert all(np.all(np.isnan(a)) for a in got[1:])
    rc[:] = 2  # finite weights, but no trajectory succeeded
    got = emulate(mean, cov, rc, np.zeros(70), 2, 2)
    assert got[0].tolist() == [0, 0] and all(np.all(np.isnan(a)) for a in got[1:])


def test_the_maximum_does_not_depend_on_the_grid_of_its_kernel():
    mean, cov, rc = make_records(2500, 1, 2, 2, seed=9)
    logw = realistic(2500, np.random.default_rng(1))
    a = emulate(mean, cov, rc, logw, 2, 8, max_blocks=1024)
    b = emulate(mean, cov, rc, logw, 2, 8, max_blocks=3)  # the lanes stride over the trajectories
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_stand_alone_program_is_clean_under_the_sanitizers(tmp_path):
    """The same source with -DODEF_EMUL_MAIN: its own main, AddressSanitizer + UBSan, run as a subprocess (no Python in it)."""
    exe = tmp_path / "emul_wsummary_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas", "-DODEF_EMUL_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("clean")
