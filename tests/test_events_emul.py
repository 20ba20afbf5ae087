"""Host build of the event location kernels (tests/emul/emul_events.cpp: csrc/events_kernels.h, the text the GPU runs) against the
definition (tests/_events_reference.py: bracket rule, bisection to adjacent doubles, oracle.dense_output) on records of oracle solves:
(d, q) = (1,1), (2,1), (2,3), (2,5), (3,3), (4,2); N = 1, 65, 130; fixed and adaptive grids; both sources; all three directions; K
smaller and larger than the count; per-trajectory levels; a repeated time; a planted NaN; an exact hit.  Bounds: the module docstring
of _events_reference."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _events_reference as er
from _emul import prior_tables

orc = er.orc
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emul", "emul_events.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_events.so")
        deps = [src] + glob.glob(os.path.join(ROOT, "odefilters.jl_amd", "csrc", "*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-Wno-unknown-pragmas", src, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def emulate(rec, source, c, levels, direction, K, adaptive=False):
    d, q = rec["d"], rec["q"]
    n, _, N = rec["mean"].shape
    At, Qt, QLt = prior_tables(q)
    lv = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, np.float64)))
    t = np.ascontiguousarray(rec["t"] if adaptive else rec["t"][:, 0])
    out = dict(count=np.full(N, -7, np.int32), time=np.full((K, N), -7.0), tvar=np.full((K, N), -7.0), u=np.full((K, d, N), -7.0),
               direction=np.full((K, N), -7, np.int32), save=np.full((K, N), -7, np.int32), neval=np.full((K, N), -7, np.int32))
    rc = lib().emul_events(d, q, _p(At), _p(Qt), _p(QLt), _p(rec["mean"]), _p(rec["cov"]), _p(rec["diff"]), _p(rec.get("smean")),
                           _p(rec.get("scov")), _p(t), _p(rec["nsaved"], C.c_int), int(adaptive), C.c_long(N), C.c_long(n), source, c,
                           direction, K, _p(lv), int(lv.size > 1), _p(out["count"], C.c_int), _p(out["time"]), _p(out["tvar"]),
                           _p(out["u"]), _p(out["direction"], C.c_int), _p(out["save"], C.c_int), _p(out["neval"], C.c_int))
    assert rc == 0, rc
    return out


def linear_field(d):
    """u' = p u on d components (oracle `linear`, any d)."""
    base = orc.vector_field("linear")
    p = np.array([1.1, -0.5, -0.9, 0.4][:d]) if d > 1 else np.array([-0.7])
    u0 = np.array([0.1, 1.0, 0.6, -0.8][:d]) if d > 1 else np.array([1.0])
    return orc.VectorField(f"linear{d}", base.rhs_id, d, d, base.f, base.jac, u0, p, (0.0, 1.0))


_RECORDS = {}


def records(field, alg, N, t1, dt=None, distinct=4, scale=1e-2, smoothed=True, repeat_at=(), adaptive=False):
    """Oracle records of `distinct` perturbed initial values, repeated to N trajectories (lane i holds trajectory i % distinct), computed
    once per configuration and left unchanged."""
    key = (field if isinstance(field, str) else field.name, alg.kind, alg.order, N, t1, dt, distinct, scale, smoothed, repeat_at, adaptive)
    if key not in _RECORDS:
        vf = field if not isinstance(field, str) else orc.vector_field(field)
        nd = min(N, distinct)
        u0s = orc.ensemble_u0(vf.u0, nd, scale)
        alg.smooth = smoothed
        if adaptive:
            sols = [orc.solve(vf, alg, u0=u0, tspan=(0.0, t1), adaptive=True, abstol=1e-6 * (1 + i), reltol=1e-3, dt=1e-2)
                    for i, u0 in enumerate(u0s)]
        else:
            sols = [orc.solve(vf, alg, u0=u0, tspan=(0.0, t1), dt=dt) for u0 in u0s]
        rec = er.records_of([sols[i % nd] for i in range(N)], smoothed=smoothed, repeat_at=repeat_at)
        rec["twin"] = np.arange(N) % nd
        _RECORDS[key] = rec
    return _RECORDS[key]


def twins(rec, levels):
    """per lane the first lane with the same records and level"""
    N = rec["nsaved"].size
    lv = np.broadcast_to(np.asarray(levels, float), (N,))
    first = {}
    return np.array([first.setdefault((int(rec["twin"][i]), float(lv[i])), i) for i in range(N)])


def run(name, rec, source, c, levels, direction, K, adaptive=False):
    out = emulate(rec, source, c, levels, direction, K, adaptive)
    stats = {}
    er.check(rec, out, c, levels, direction, K, bool(source), label=name, stats=stats, same_as=twins(rec, levels))
    print(name, er.summarize(stats))
    again = emulate(rec, source, c, levels, direction, K, adaptive)
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in er.KEYS)  # bit for bit
    return out


LV = dict(field="lotka_volterra", t1=6.0, dt=2.0 ** -4)
CASES = {
    # name: (records, source, component, level(s), direction, K)
    "lin1-ek0q1-N1": (dict(field=linear_field(1), alg=orc.EK0(order=1), N=1, t1=1.0, dt=2.0 ** -4), 0, 0, 0.7, 0, 2),
    "lin1-ek0q1-N1-smooth": (dict(field=linear_field(1), alg=orc.EK0(order=1), N=1, t1=1.0, dt=2.0 ** -4), 1, 0, 0.7, -1, 1),
    "fhn-ek1q1-N65-up": (dict(field="fhn", alg=orc.EK1(order=1), N=65, t1=3.0, dt=2.0 ** -4), 0, 0, 0.0, 1, 2),
    "lv-ek1q3-N130-K2-truncated": (dict(alg=orc.EK1(order=3), N=130, **LV), 1, 1, 1.0, 0, 2),
    "lv-ek1q3-N130-K6-filter": (dict(alg=orc.EK1(order=3), N=130, **LV), 0, 1, 1.0, 0, 6),
    "lv-ek1q3-N65-down-pertraj": (dict(alg=orc.EK1(order=3), N=65, **LV), 1, 1, "pertraj", -1, 3),
    "lv-ek1q3-N65-repeat": (dict(alg=orc.EK1(order=3), N=65, repeat_at=(20, 47), **LV), 1, 1, 1.0, 0, 4),
    "vdp-ek1q5-N65": (dict(field="vanderpol", alg=orc.EK1(order=5), N=65, t1=6.25, dt=2.0 ** -4), 1, 0, 0.5, 0, 3),
    "lorenz-ek1q3-N130": (dict(field="lorenz63", alg=orc.EK1(order=3), N=130, t1=1.0, dt=2.0 ** -6), 1, 0, 0.0, 0, 2),
    "lorenz-ek1q3-N65-filter-pertraj": (dict(field="lorenz63", alg=orc.EK1(order=3), N=65, t1=1.0, dt=2.0 ** -6), 0, 0, "pertraj", -1, 1),
    "lin4-ek0q2-N65": (dict(field=linear_field(4), alg=orc.EK0(order=2), N=65, t1=1.0, dt=2.0 ** -4, scale=1e-3), 1, 0, 0.2, 0, 2),
    "lv-ek1q3-N65-adaptive": (dict(field="lotka_volterra", alg=orc.EK1(order=3), N=65, t1=6.0, adaptive=True, repeat_at=(9,)), 1, 1, 1.0,
                              0, 5),
    "lv-ek1q3-N130-adaptive-filter": (dict(field="lotka_volterra", alg=orc.EK1(order=3), N=130, t1=6.0, adaptive=True), 0, 1, "pertraj",
                                      1, 1),
}


def _levels(spec, N, base):
    if not isinstance(spec, str):
        return spec
    return base + 0.01 * (np.arange(N) % 7 - 3)  # seven levels against four distinct trajectories: 28 different problems


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_pass_on_oracle_records(name):
    kw, source, c, level, direction, K = CASES[name]
    rec = records(**kw)
    lv = _levels(level, kw["N"], 1.0 if "lv" in name else 0.0)
    out = run(name, rec, source, c, lv, direction, K, adaptive=kw.get("adaptive", False))
    assert out["count"].max() >= 1, "a case without an event checks nothing"
    if "truncated" in name:
        assert np.all(out["count"] == 4) and K == 2           # Lotka-Volterra above has four crossings
    if "K6" in name:
        assert np.all(out["count"] == 4) and np.all(out["save"][4:] == -1)


def test_every_pair_and_size_is_run():
    pairs = {(r["field"].d if not isinstance(r["field"], str) else orc.vector_field(r["field"]).d, r["alg"].order)
             for r, *_ in CASES.values()}
    assert pairs == {(1, 1), (2, 1), (2, 3), (2, 5), (3, 3), (4, 2)}
    assert {r["N"] for r, *_ in CASES.values()} == {1, 65, 130}
    assert {c[4] for c in CASES.values()} == {-1, 0, 1} and {c[1] for c in CASES.values()} == {0, 1}


def test_a_repeated_time_holds_no_event():
    """A record planted again at the unchanged time INSIDE a bracket: the zero-length interval is no event, the count is unchanged and
    the bracket moves to the copy (whose successor lies later)."""
    plain = records(alg=orc.EK1(order=3), N=65, **LV)
    ref = emulate(plain, 1, 1, 1.0, 0, 4)
    k0 = int(ref["save"][0, 0])
    rec = records(alg=orc.EK1(order=3), N=65, repeat_at=(k0,), **LV)
    out = run("repeat-in-bracket", rec, 1, 1, 1.0, 0, 4)
    same = ref["save"][0] == k0                              # the lanes whose first bracket starts at that save
    assert same.sum() >= 16 and np.array_equal(out["count"], ref["count"]) and np.all(out["save"][0][same] == k0 + 1)
    assert np.array_equal(out["time"][0][same], ref["time"][0][same])


def test_a_nan_stays_in_its_lane():
    base = records(alg=orc.EK1(order=3), N=130, **LV)
    ref = emulate(base, 1, 1, 1.0, 0, 4)
    rec = dict(base)
    rec["smean"] = base["smean"].copy()
    k = int(ref["save"][1, 7])
    rec["smean"][k + 1, 1, 7] = np.nan                      # the right end of trajectory 7's second bracket
    lv = np.full(130, 1.0)
    lv[70] = np.nan                                          # a NaN level: no event at all
    out = emulate(rec, 1, 1, lv, 0, 4)
    assert out["count"][70] == 0 and np.all(out["save"][:, 70] == -1) and np.all(np.isnan(out["time"][:, 70]))
    assert out["count"][7] == ref["count"][7] - 1           # neither interval that touches the NaN holds an event
    assert np.array_equal(out["time"][1:3, 7], ref["time"][2:4, 7])
    others = np.setdiff1d(np.arange(130), [7, 70])
    for key in er.KEYS:
        assert np.array_equal(out[key][..., others], ref[key][..., others], equal_nan=True), key


@pytest.mark.parametrize("source", [0, 1])
def test_an_exact_hit_returns_the_stored_record(source):
    """The level set per trajectory to the stored mean of save k + 1 of its first bracket: t* = t_{k+1}, the outputs are the stored
    record bit for bit, NEVAL = 0, and the interval that starts at g = 0 is no bracket."""
    rec = records(alg=orc.EK1(order=3), N=65, **LV)
    ref = emulate(rec, source, 1, 1.0, 0, 4)
    N = 65
    k1 = ref["save"][0].astype(int) + 1
    mean = rec["smean"] if source else rec["mean"]
    cov = rec["scov"] if source else rec["cov"]
    lv = mean[k1, 1, np.arange(N)].copy()
    out = emulate(rec, source, 1, lv, 0, 4)
    ii = np.arange(N)
    assert np.array_equal(out["save"][0], ref["save"][0]) and np.all(out["neval"][0] == 0) and np.all(out["count"] == 4)
    assert np.array_equal(out["time"][0], rec["t"][k1, ii])
    assert np.array_equal(out["u"][0], mean[k1, :2, ii].T)
    tri_cc = 1 * 2 // 2 + 1
    assert np.array_equal(out["tvar"][0], cov[k1, tri_cc, ii] / (mean[k1, 2 + 1, ii] * mean[k1, 2 + 1, ii]))
    assert np.all(out["neval"][1:4] >= 1)
    er.check(rec, out, 1, lv, 0, 4, bool(source), label="exact", same_as=twins(rec, lv))


def test_a_crossing_inside_the_measurement_update():
    """Filter source: the level set per trajectory between the left limit of the interpolant at a save (the prediction from the save
    before) and the stored mean there.  The stored means bracket the level, the interpolant has no root: the event is the save, the
    outputs are its stored record bit for bit, NEVAL = 1 (the left limit)."""
    rec = records(alg=orc.EK1(order=3), N=65, **LV)
    N, ii = 65, np.arange(65)
    lv, ks = np.zeros(N), np.zeros(N, int)
    for i in range(4):                                       # the four distinct trajectories
        sol = er.trajectory(rec, i)
        consts = orc.make_consts(sol.d, sol.q)
        for k in range(8, len(sol.t) - 1):
            lim, a, b = er.left_limit(sol, consts, k)[1], sol.x_filt[k].mu[1], sol.x_filt[k + 1].mu[1]
            if (a < lim < b or a > lim > b) and abs(b - lim) > 1e-9:
                lv[i::4], ks[i::4] = 0.5 * (lim + b), k
                break
        else:
            raise AssertionError("no save whose update continues the step's direction")
    out = emulate(rec, 0, 1, lv, 0, 8)
    hit = np.argmax(out["save"] == ks[None, :], axis=0)
    assert np.all(out["save"][hit, ii] == ks) and np.all(out["neval"][hit, ii] == 1)
    assert np.array_equal(out["time"][hit, ii], rec["t"][ks + 1, 0])
    assert np.array_equal(out["u"][hit, :, ii], rec["mean"][ks + 1, :2, ii])
    assert np.array_equal(out["tvar"][hit, ii], rec["cov"][ks + 1, 2, ii] / (rec["mean"][ks + 1, 3, ii] * rec["mean"][ks + 1, 3, ii]))
    stats = {}
    er.check(rec, out, 1, lv, 0, 8, False, label="update", stats=stats, same_as=twins(rec, lv))
    assert stats["jumps"] >= 4                                # (a level may meet another update by itself)
    smooth = emulate(rec, 1, 1, lv, 0, 8)                    # the smoothed interpolant is continuous: every bracket has its root
    er.check(rec, smooth, 1, lv, 0, 8, True, label="update, smoothed", stats=(st := {}), same_as=twins(rec, lv))
    assert "jumps" not in st


def test_a_pair_without_an_instance_is_refused():
    z, i4 = np.zeros(64), np.zeros(4, np.int32)
    At, Qt, QLt = prior_tables(5)
    for d, q in ((3, 4), (4, 3), (5, 1), (2, 6), (1, 0)):
        assert lib().emul_events(d, q, _p(At), _p(Qt), _p(QLt), _p(z), _p(z), _p(z), _p(z), _p(z), _p(z), _p(i4, C.c_int), 0, C.c_long(1),
                                 C.c_long(2), 0, 0, 0, 1, _p(z), 0, _p(i4, C.c_int), _p(z), _p(z), _p(z), _p(i4, C.c_int), _p(i4, C.c_int),
                                 _p(i4, C.c_int)) == -1, (d, q)
