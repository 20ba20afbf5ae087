"""The reference of the event location tests (tests/_events_reference.py) is the right quantity: (a) the slope the Newton iteration
uses, E[u'_c(t)] = mean entry d + c of the dense posterior, is the derivative of the dense mean E[u_c(t)] (central difference, step
1e-6, to 1e-5 relative) for the filter and the smoothed interpolant; (b) the restated Newton iteration and plain bisection find the
same root within the time bound; (c) the located times are calibrated: the DOP853 events (rtol = atol = 1e-12) of eight perturbed
trajectories each of van der Pol, Lotka-Volterra and Lorenz-63 under EK1(3) are as many as the located ones and lie within 3 reported
standard deviations of them (the reference's worst is 0.70)."""
import numpy as np
import pytest
from scipy.integrate import solve_ivp

import _events_reference as er

orc = er.orc

# field, component, level, dt, t1, ensemble_u0 scale
FIELDS = {
    "vanderpol": (0, 0.5, 2.0 ** -4, 6.25, 1e-1),
    "lotka_volterra": (1, 1.0, 2.0 ** -4, 6.0, 1e-1),
    "lorenz63": (0, 0.0, 2.0 ** -6, 1.0, 1e-2),
}
_SOLS = {}


def solutions(name, n=8):
    if name not in _SOLS:
        c, level, dt, t1, scale = FIELDS[name]
        vf = orc.vector_field(name)
        u0s = orc.ensemble_u0(vf.u0, n, scale)
        _SOLS[name] = (vf, u0s, [orc.solve(vf, orc.EK1(order=3, smooth=True), u0=u0, tspan=(0.0, t1), dt=dt) for u0 in u0s])
    return _SOLS[name]


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("smoothed", [False, True])
def test_the_slope_is_the_derivative_of_the_dense_mean(name, smoothed):
    c, level, dt, t1, _ = FIELDS[name]
    _, _, sols = solutions(name)
    sol = sols[0]
    consts = orc.make_consts(sol.d, sol.q)
    worst = 0.0
    for frac in (0.137, 0.5, 0.861):
        for k in (1, len(sol.t) // 2, len(sol.t) - 2):
            t = sol.t[k] + frac * (sol.t[k + 1] - sol.t[k])
            e = 1e-6
            fd = (er.dense(sol, consts, t + e, smoothed).mu[: sol.d] - er.dense(sol, consts, t - e, smoothed).mu[: sol.d]) / (2 * e)
            slope = er.dense(sol, consts, t, smoothed).mu[sol.d: 2 * sol.d]
            worst = max(worst, float(np.max(np.abs(fd - slope) / np.maximum(np.abs(slope), 1e-3))))
    print(name, "smoothed" if smoothed else "filter", "slope against central difference, worst relative", f"{worst:.2e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("name", list(FIELDS))
def test_newton_and_bisection_find_the_same_root(name):
    c, level, dt, t1, _ = FIELDS[name]
    _, _, sols = solutions(name)
    worst, counts = 0.0, []
    for sol in sols[:4]:
        for smoothed in (False, True):
            ref = er.locate(sol, c, level, 0, 8, smoothed)
            assert ref["count"] >= 1
            for e in ref["events"]:
                tn, nev = er.newton(sol, ref["consts"], c, level, e["k"], smoothed)
                bound = e["eps"] / abs(e["slope"]) + 4 * np.spacing(abs(e["t"]))
                worst = max(worst, abs(tn - e["t"]) / bound)
                counts.append(nev)
    print(name, "Newton against bisection: worst share of the time bound", f"{worst:.2e}", "evaluations max", max(counts), "median",
          int(np.median(counts)))
    assert worst <= 1.0 and max(counts) <= er.MAX_EVAL


@pytest.mark.parametrize("name", list(FIELDS))
def test_located_times_are_calibrated_against_dop853(name):
    c, level, dt, t1, _ = FIELDS[name]
    vf, u0s, sols = solutions(name)

    def ev(t, u):
        return u[c] - level

    worst = 0.0
    for u0, sol in zip(u0s, sols):
        truth = solve_ivp(lambda t, u: vf.f(u, vf.p, t), (0.0, t1), u0, method="DOP853", rtol=1e-12, atol=1e-12, events=ev)
        te = truth.t_events[0]
        ref = er.locate(sol, c, level, 0, 16, True)
        assert ref["count"] == len(te) >= 1, (name, ref["count"], len(te))
        for e, tt in zip(ref["events"], te):
            std = np.sqrt(e["tvar"])
            assert abs(e["slope"]) >= 0.5
            worst = max(worst, abs(e["t"] - tt) / std)
    print(name, "true crossing within", f"{worst:.2f}", "reported standard deviations of the located one (worst)")
    assert worst <= 3.0
