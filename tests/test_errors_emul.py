"""Host build of the solution-error kernels (tests/emul/emul_errors.cpp: csrc/errors_kernels.h) against the extended-precision
reference (tests/_errors_reference.py): oracle solutions of the linear problem on a fixed grid and adaptive with a planted
zero-length repeat, filter and smoothed, the truth from `RhsLinear::analytic` and from a buffer; random records for d = 1, 2, 3, 16,
28 with ragged last workgroups; every number of time chunks the launcher can choose; zero-covariance records, a semi-definite
block, NaN trajectories.  The tolerances are 16 times the measured error of the plain numpy float64 evaluation, in units of the
bounds derived in `_errors_reference.unit_bounds`.  ODEF_EMUL_SANITIZE=1 builds with AddressSanitizer + UBSan
(tools/sanitize_emul.sh)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _errors_reference as er
from _errors_reference import orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        san = os.environ.get("ODEF_EMUL_SANITIZE") == "1"
        src = os.path.join(HERE, "emul", "emul_errors.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_errors_san.so" if san else "libodef_emul_errors.so")
        csrc = os.path.join(ROOT, "odefilters.jl_amd", "csrc")
        deps = [src, os.path.join(csrc, "rhs.h"), os.path.join(csrc, "odef_platform.h")] + glob.glob(os.path.join(csrc, "errors*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else []
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-Wno-unknown-pragmas"] + flags + [src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.emul_errors_split.argtypes = [C.c_long, C.c_long, C.c_int]
    return _LIB


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def emulate(mean, cov, d, truth=None, tsave=None, nsaved=None, n_split=0, linear=None):
    """The five arrays from the host build; truth: buffer [n_save, d, N], or linear = (u0 [N, 2], p, t) for RhsLinear::analytic."""
    n_save, D, N = mean.shape
    TRI = cov.shape[1]
    mean, cov = np.ascontiguousarray(mean), np.ascontiguousarray(cov)
    out = [np.full(N, -7.0) for _ in range(4)]
    nused = np.full(N, -7, np.int64)
    ts = None if nsaved is None else np.ascontiguousarray(tsave)
    ns = None if nsaved is None else np.ascontiguousarray(nsaved, np.int32)
    if linear is None:
        tr = np.ascontiguousarray(truth, np.float64)
        s = lib().emul_errors(n_split, _p(mean), _p(cov), _p(ts), _p(ns, C.c_int), _p(tr), C.c_long(N), C.c_long(n_save), d, D, TRI,
                              *[_p(o) for o in out], _p(nused, C.c_longlong))
    else:
        u0, p, t = linear
        u0d = np.ascontiguousarray(np.asarray(u0, float).T)  # [d][N]
        p = np.asarray(p, float)
        shared = p.ndim == 1
        pd = np.ascontiguousarray(p if shared else p.T)
        t = np.ascontiguousarray(t, float)
        sk, si = (1, 0) if t.ndim == 1 else (N, 1)
        s = lib().emul_errors_linear(n_split, _p(mean), _p(cov), _p(ts), _p(ns, C.c_int), _p(u0d), _p(pd), int(shared), _p(t),
                                     C.c_long(sk), C.c_long(si), C.c_long(N), C.c_long(n_save), D, TRI, *[_p(o) for o in out],
                                     _p(nused, C.c_longlong))
    return dict(zip(er.KEYS, out), nused=nused), s


def random_records(d, q, N, n_save, seed, adaptive=False):
    """Records whose solution block is B B' (B of d x (d + 2) normals, times 1e-6) and whose error is e = B z: chi2 ~ 1.  Record 0
    has a zero block, as the initial record; trajectory 1 is all zero blocks (chi2 NaN); trajectory 2 (d >= 2) has a block whose
    first variable carries no uncertainty at save 2 (a zero pivot); trajectory 3 has a NaN mean at save 1, trajectory 4 a NaN
    covariance entry at save 1."""
    rng = np.random.default_rng(seed)
    D = d * (q + 1)
    TRI = D * (D + 1) // 2
    mean = rng.uniform(-3.0, 3.0, (n_save, D, N))
    cov = rng.uniform(-1e-7, 1e-7, (n_save, TRI, N))
    B = 1e-3 * rng.standard_normal((n_save, N, d, d + 2))
    S = B @ B.transpose(0, 1, 3, 2)
    e = (B @ rng.standard_normal((n_save, N, d + 2, 1)))[..., 0]  # [n_save, N, d]
    if N > 2 and d >= 2 and n_save > 2:
        S[2, 2, 0, :] = S[2, 2, :, 0] = 0.0
    for a in range(d):
        for b in range(a + 1):
            cov[:, a * (a + 1) // 2 + b, :] = S[:, :, a, b]
    cov[0, : er.tri(d), :] = 0.0
    if N > 1:
        cov[:, : er.tri(d), 1] = 0.0
    truth = mean[:, :d, :] - e.transpose(0, 2, 1)
    if N > 4 and n_save > 1:
        mean[1, d - 1, 3] = np.nan
        cov[1, 0, 4] = np.nan
    tsave = nsaved = None
    if adaptive:
        nsaved = rng.integers(2, n_save + 1, N).astype(np.int32)
        nsaved[0] = n_save
        tsave = np.cumsum(rng.uniform(0.01, 0.1, (n_save, N)), axis=0)
        rep = rng.random((n_save, N)) < 0.15  # rejected attempts: the record again at the unchanged time
        rep[:2] = False
        for k in range(1, n_save):
            tsave[k] = np.where(rep[k], tsave[k - 1], tsave[k])
        tsave = np.maximum.accumulate(tsave, axis=0)
    return mean, cov, truth, tsave, nsaved


RANDOM = [  # d, q, N, n_save, adaptive
    (1, 3, 70, 9, False), (2, 2, 300, 12, True), (3, 3, 257, 17, False), (3, 1, 63, 40, True), (8, 1, 20, 6, False),
    (9, 1, 70, 5, True), (16, 1, 70, 6, False), (16, 1, 33, 7, True), (22, 0, 17, 4, False), (28, 1, 21, 5, False), (28, 0, 9, 6, True),
    (32, 0, 9, 3, False),
]


def _linear_cases():
    vf = orc.vector_field("linear")
    u0s = orc.ensemble_u0(vf.u0, 5, 1e-2)
    out = []
    tg = np.arange(13) * 2.0 ** -4
    for alg, sm in ((orc.EK0(order=2, smooth=True), False), (orc.EK1(order=3, smooth=True), True)):
        mean, cov, t, _ = er.oracle_records(vf, alg, u0s, tgrid=tg, smoothed=sm)
        out.append((f"fixed-{alg.kind}{alg.order}-{'smooth' if sm else 'filter'}", mean, cov, t, None, u0s, vf.p))
    ad = dict(t1=1.0, dt0=2.0 ** -6, abstol=1e-6, reltol=1e-4)
    for alg, sm in ((orc.EK1(order=3, smooth=True), False), (orc.EK0(order=3, smooth=True), True)):
        mean, cov, ts, ns = er.oracle_records(vf, alg, u0s, adaptive=ad, smoothed=sm, repeat_at=(2, 5))
        out.append((f"adaptive-{alg.kind}{alg.order}-{'smooth' if sm else 'filter'}", mean, cov, ts, ns, u0s, vf.p))
    return out


_LIN = None


def linear_cases():
    global _LIN
    if _LIN is None:
        _LIN = _linear_cases()
    return _LIN


def test_float64_numpy_evaluation_calibrates_the_tolerances():
    """The numpy float64 evaluation of the definitions against the longdouble reference on every input of this file, in units of
    `unit_bounds`: the measured constants C_NUMPY are not exceeded (the device gets 16 times them)."""
    worst = dict.fromkeys(er.KEYS, 0.0)
    for (d, q, N, n_save, ad) in RANDOM:
        mean, cov, truth, ts, ns = random_records(d, q, N, n_save, 100 * d + N, ad)
        ref = er.evaluate(mean, cov, d, truth, ts, ns)
        f64 = er.evaluate(mean, cov, d, truth, ts, ns, dtype=np.float64)
        r = er.ratios(f64, ref, er.unit_bounds(mean, cov, d, truth, ref, ts, ns))
        worst = {k: max(worst[k], r[k]) for k in er.KEYS}
    for (label, mean, cov, ts, ns, u0s, p) in linear_cases():
        tl = er.linear_truth(u0s, p, ts)
        ref = er.evaluate(mean, cov, 2, tl, ts if ns is not None else None, ns)
        f64 = er.evaluate(mean, cov, 2, er.linear_truth(u0s, p, ts, np.float64), ts if ns is not None else None, ns, dtype=np.float64)
        r = er.ratios(f64, ref, er.unit_bounds(mean, cov, 2, tl, ref, ts if ns is not None else None, ns))
        print(label, {k: f"{v:.3g}" for k, v in r.items()})
        worst = {k: max(worst[k], r[k]) for k in er.KEYS}
    print("numpy float64 / unit bound, worst:", {k: f"{v:.3g}" for k, v in worst.items()})
    for k in er.KEYS:
        assert worst[k] <= er.C_NUMPY[k], (k, worst[k])


@pytest.mark.parametrize("d,q,N,n_save,adaptive", RANDOM, ids=[f"d{c[0]}-N{c[2]}-n{c[3]}-{'ad' if c[4] else 'fx'}" for c in RANDOM])
def test_emulated_errors_on_random_records(d, q, N, n_save, adaptive):
    mean, cov, truth, ts, ns = random_records(d, q, N, n_save, 100 * d + N, adaptive)
    ref = er.evaluate(mean, cov, d, truth, ts, ns)
    bounds = er.unit_bounds(mean, cov, d, truth, ref, ts, ns)
    got, s = emulate(mean, cov, d, truth, ts, ns)
    assert s == lib().emul_errors_split(N, n_save, d)
    r = er.check(got, ref, bounds, label=f"d={d} N={N}")
    print(f"d={d} N={N} n_save={n_save} chunks={s} lanes={lib().emul_errors_lanes(d)}: error / unit bound", {k: f"{v:.3g}" for k, v in r.items()})
    if N > 4:
        assert np.isnan(got["chi2"][1]) and got["nused"][1] > 0 and np.isfinite(got["l2"][1])  # every block zero: chi2 NaN, not 0
        assert np.isnan(got["l2"][3]) and np.isnan(got["linf"][3])                              # a NaN mean propagates
        assert np.isnan(got["chi2"][4]) and np.isfinite(got["l2"][4])                           # a NaN covariance: chi2 only
    if adaptive:
        used = er.used_mask(n_save, N, ts, ns)
        assert np.array_equal(got["nused"], used.sum(axis=0)) and np.any(got["nused"] < ns)


@pytest.mark.parametrize("n_save,want", [(8, 1), (16, 2), (32, 4), (64, 8), (128, 16), (256, 32), (512, 64), (1025, 64)])
def test_every_number_of_time_chunks_the_launcher_chooses(n_save, want):
    """One workgroup of trajectories: the launcher doubles the chunks while a chunk keeps 8 saves, up to 64.  Every choice
    gives the reference's numbers, fixed grid and adaptive; so does every forced count on a short record (empty chunks)."""
    d, N = 3, 40
    assert lib().emul_errors_split(N, n_save, d) == want
    for adaptive in (False, True):
        mean, cov, truth, ts, ns = random_records(d, 0, N, n_save, n_save + adaptive, adaptive)
        ref = er.evaluate(mean, cov, d, truth, ts, ns)
        got, s = emulate(mean, cov, d, truth, ts, ns)
        assert s == want
        er.check(got, ref, er.unit_bounds(mean, cov, d, truth, ref, ts, ns), label=f"n_save={n_save}")
    if n_save == 16:
        for forced in (1, 2, 4, 8, 16, 32, 64):
            got, s = emulate(mean, cov, d, truth, ts, ns, n_split=forced)
            assert s == forced
            er.check(got, ref, er.unit_bounds(mean, cov, d, truth, ref, ts, ns), label=f"forced {forced}")


def test_grid_covers_the_device_at_the_headline_sizes():
    L = lib()
    assert L.emul_errors_lanes(3) == 256 and L.emul_errors_lanes(8) == 256
    assert [L.emul_errors_lanes(d) for d in (9, 14, 15, 21, 22, 28, 30, 31, 32)] == [64, 64, 32, 32, 16, 16, 16, 8, 8]
    for d in range(9, 33):
        assert (er.tri(d) + d) * L.emul_errors_lanes(d) * 8 <= 65536
    assert L.emul_errors_split(65536, 1025, 3) == 4      # 256 blocks of trajectories x 4 chunks = 1 024 workgroups
    assert L.emul_errors_split(4096, 1025, 3) == 64      # 16 x 64
    assert L.emul_errors_split(65536, 1, 3) == 1         # final-save mode


@pytest.mark.parametrize("k", range(4))
def test_emulated_errors_of_oracle_solutions_of_the_linear_problem(k):
    """Truth from RhsLinear::analytic in the kernel (float64 exp) and from a buffer, against u0 exp(p t) in longdouble."""
    label, mean, cov, ts, ns, u0s, p = linear_cases()[k]
    ad_t = ts if ns is not None else None
    tl = er.linear_truth(u0s, p, ts)
    ref = er.evaluate(mean, cov, 2, tl, ad_t, ns)
    bounds = er.unit_bounds(mean, cov, 2, tl, ref, ad_t, ns)
    got, _ = emulate(mean, cov, 2, tsave=ad_t, nsaved=ns, linear=(u0s, p, ts))
    r = er.check(got, ref, bounds, label=label)
    print(label, "analytic: error / unit bound", {k: f"{v:.3g}" for k, v in r.items()})
    got_b, _ = emulate(mean, cov, 2, truth=tl.astype(np.float64), tsave=ad_t, nsaved=ns)
    er.check(got_b, ref, bounds, label=label + " buffer")
    if ns is not None:  # two planted repeats per trajectory: NUSED = accepted steps + 1
        assert np.array_equal(got["nused"], ns - 2)
        assert np.all(got["nused"] >= 3)
    else:
        assert np.all(got["nused"] == mean.shape[0])
    assert np.all(got["l2"] > 0) and np.all(got["final"] > 0) and np.all(got["chi2"] > 0)


def test_emulated_truth_kernel():
    label, mean, cov, ts, ns, u0s, p = linear_cases()[2]
    n_save, _, N = mean.shape
    out = np.full((n_save, 2, N), -7.0)
    u0d, pd, t = np.ascontiguousarray(np.asarray(u0s).T), np.ascontiguousarray(p, float), np.ascontiguousarray(ts)
    lib().emul_truth_linear(_p(np.ascontiguousarray(ns, np.int32), C.c_int), _p(u0d), _p(pd), 1, _p(t), C.c_long(N), C.c_long(1),
                            C.c_long(N), C.c_long(n_save), _p(out))
    want = er.linear_truth(u0s, p, ts)
    live = np.arange(n_save)[:, None] < ns[None, :]
    assert np.all(out[~np.broadcast_to(live[:, None, :], out.shape)] == 0.0)
    m = np.broadcast_to(live[:, None, :], out.shape)
    assert np.all(np.abs(out[m] - want[m].astype(float)) <= 4 * er.U * np.abs(want[m].astype(float)))
