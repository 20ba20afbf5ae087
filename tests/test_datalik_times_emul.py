"""Host build of the kernel of the data log-likelihood at arbitrary times (tests/emul/emul_datalik_times.cpp:
csrc/datalik_times_kernels.h) against the extended-precision reference of the augmented chain (tests/_datalik_times_reference.py)
on records of oracle solves: (d, q) = (1,1), (2,1), (2,3), (2,5), (3,3), (4,2); N = 1, 65, 130; fixed grids of 5 to 33 saves and
ragged per-trajectory grids of adaptive solves with planted repeats; two and three times inside one step, times on saves, at save
0 and at the shared last save, nextafter above and below a save, all times inside the first / the last step; o < d and o = d;
about one time per step, each 1e-6 to 1e-3 of the
step above a save; shared and per-trajectory values; dynamic, fixed and fixedMAP diffusion; a NaN planted in one lane's record; lanes whose records
end before the last time.  Bound: 16 C_NUMPY unit_bound (`_datalik_times_reference.check`)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _datalik_times_reference as tr
from _emul import prior_tables

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emul", "emul_datalik_times.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_datalik_times.so")
        deps = [src] + glob.glob(os.path.join(ROOT, "odefilters.jl_amd", "csrc", "*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-Wno-unknown-pragmas", src, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def emulate(c, wave=64):
    mean, cov, diff = (np.ascontiguousarray(c[k], np.float64) for k in ("mean", "cov", "diff"))
    n, _, N = mean.shape
    At, Qt, QLt = prior_tables(c["q"])
    times, comps = np.ascontiguousarray(c["times"], np.float64), np.ascontiguousarray(c["comps"], np.int64)
    y = np.asarray(c["y"], np.float64)
    per_traj = y.ndim == 3
    val = np.ascontiguousarray(y.transpose(1, 2, 0) if per_traj else y)  # [M][o][N] or [M][o]
    r, t = np.ascontiguousarray(c["r"], np.float64), np.ascontiguousarray(c["t"], np.float64)
    adaptive = c["nsaved"] is not None
    ns = np.ascontiguousarray(c["nsaved"], np.int32) if adaptive else None
    ll, mq = np.full(N, -7.0), np.full(N, -7.0)
    rc = lib().emul_datalik_times(c["d"], c["q"], _p(At), _p(Qt), _p(QLt), _p(mean), _p(cov), _p(diff), int(adaptive),
                                  None if adaptive else _p(t), _p(t) if adaptive else None, _p(ns, C.c_int) if adaptive else None,
                                  C.c_long(N), C.c_long(n), _p(times), len(times), _p(comps, C.c_longlong), len(comps), _p(val),
                                  int(per_traj), _p(r), wave, _p(ll), _p(mq))
    assert rc == 0, rc
    return {"loglik": ll, "mahalanobis": mq}


NAMES = ["lin1-ek0q1-N1-mixed", "fhn-ek1q1-fixed-N65-three-in-step", "lv-ek0q3-N130-all-in-first-step",
         "lv-ek1q3-map-N65-all-in-last-step", "lin4-ek0q2-N65-mixed-pertraj", "fhn-ek1q1-N65-repeat", "lorenz-ek1q3-N130-ragged",
         "fhn-ek0q5-N65-ragged-pertraj", "lv-ek0q3-map-N65-ragged", "lorenz-ek1q3-N65-ragged-short",
         "lorenz-ek1q3-N65-ragged-above-saves", "fhn-ek0q5-N65-ragged-above-saves"]


@pytest.mark.parametrize("name", NAMES)
def test_emulated_pass_on_oracle_records(name):
    c = tr.cases()[name]
    ref = tr.run_reference(c)
    got = emulate(c)
    r = tr.check(got, ref, tr.case_bound(c), label=name)
    print(name, "error / unit bound", {k: f"{v:.3g}" for k, v in r.items()}, "allowed", tr.DEVICE_FACTOR * tr.C_NUMPY)
    fin = np.isfinite(got["loglik"])
    if name.endswith("short"):  # the lanes whose records end before the last time, and only they
        assert list(np.flatnonzero(~fin)) == list(range(1, 65, 5))
    else:
        assert np.all(fin)
    assert np.all(got["mahalanobis"][fin] >= 0)
    # bit for bit again, and with every lane a wavefront of its own (no lane joins below the start of the walk)
    for again in (emulate(c), emulate(c, wave=1)):
        assert all(got[k].tobytes() == again[k].tobytes() for k in tr.KEYS)


def test_every_case_of_the_reference_is_run():
    assert sorted(NAMES) == sorted(tr.cases())
    pairs = {(c["d"], c["q"]) for c in tr.cases().values()}
    assert pairs == {(1, 1), (2, 1), (2, 3), (2, 5), (3, 3), (4, 2)}
    assert {c["mean"].shape[-1] for c in tr.cases().values()} == {1, 65, 130}


def test_ragged_grids_differ_per_lane():
    c = tr.cases()["lorenz-ek1q3-N130-ragged"]
    assert len(set(c["nsaved"][:5])) > 1 and c["mean"].shape[0] > c["nsaved"].max()
    t0 = c["t"][: c["nsaved"][0], 0]
    assert np.any(np.diff(t0) == 0)                         # the planted repeats


def test_a_nan_in_one_record_stays_in_its_lane():
    for name, (k1, i1), (k2, i2) in (("lorenz-ek1q3-N130-ragged", (6, 7), (3, 70)), ("fhn-ek1q1-N65-repeat", (9, 7), (5, 33))):
        c = dict(tr.cases()[name])
        c["mean"], c["cov"] = c["mean"].copy(), c["cov"].copy()
        c["mean"][k1, 1, i1] = np.nan     # a swept record of one trajectory
        c["cov"][k2, 2, i2] = np.nan      # a covariance entry of another
        ref, got = tr.run_reference(c), emulate(c)
        bad = np.isnan(got["loglik"])
        assert list(np.flatnonzero(bad)) == [i1, i2] and np.array_equal(bad, np.isnan(got["mahalanobis"]))
        tr.check(got, ref, tr.case_bound(c), label="nan")


def test_on_grid_times_agree_with_the_save_path_reference():
    """All times on saves: the augmented chain is the records, and the time-path kernel meets the save-path reference."""
    import _datalik_reference as dr

    c = dr.cases()["lorenz-ek1q3-N130-c02-4th"]
    ct = dict(c, times=np.asarray(c["t"])[c["saves"]], nsaved=None)
    got = emulate(ct)
    dr.check(got, dr.run_reference(c), dr.case_bound(c), label="on grid")


def test_a_pair_without_an_instance_is_refused():
    z = np.zeros(8)
    i8 = np.zeros(1, np.int64)
    At, Qt, QLt = prior_tables(3)
    assert lib().emul_datalik_times(4, 3, _p(At), _p(Qt), _p(QLt), _p(z), _p(z), _p(z), 0, _p(z), None, None, C.c_long(1), C.c_long(2),
                                    _p(z), 1, _p(i8, C.c_longlong), 1, _p(z), 0, _p(z), 1, _p(z), _p(z)) == -1
