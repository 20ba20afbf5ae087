"""The reference for time-dependent fields (tests/_time_reference.py) pinned on the CPU: the wrapped field's Taylor
initialisation against hand-written total derivatives, and the convergence orders of the fixed-grid solve against the analytic
solution (the reference's own criterion, test/convergence.jl: q + 1 within TESTTOL = 0.2)."""
import numpy as np
import pytest

import _time_reference as tr
import odefilter_oracle as orc

DTS = [2.0**-4, 2.0**-5, 2.0**-6]


def test_initialisation_carries_the_time_jet():
    vf = tr.forced()
    t0 = vf.tspan[0]
    x = orc.initial_update(vf.u0, vf, vf.p, t0, 3)
    want = np.concatenate([vf.u0] + tr.forced_derivatives(vf.u0, vf.p, t0))
    np.testing.assert_allclose(x.mu, want, rtol=1e-13, atol=0)
    assert np.abs(x.L @ x.L.T).max() < 1e-20
    # without the jet the second derivative loses f_t: the wrapper is what puts it there
    bare = orc.VectorField("bare", 7, 2, 3, tr._forced_f, tr._forced_jac, vf.u0, vf.p, vf.tspan)
    plain = orc.get_derivatives(vf.u0, bare, vf.p, t0, 2)[1]
    assert abs(plain[0] - want[4]) > 1.0 and abs(plain[1] - want[5]) > 0.5


def test_analytic_solves_the_field():
    vf = tr.forced()
    t0, h = vf.tspan[0], 1e-5
    for t in (0.25, 1.0, 2.25):
        u = tr.forced_analytic(vf.u0, vf.p, t0, t)[0]
        du = (tr.forced_analytic(vf.u0, vf.p, t0, t + h)[0] - tr.forced_analytic(vf.u0, vf.p, t0, t - h)[0]) / (2 * h)
        np.testing.assert_allclose(du, tr._forced_f(u, vf.p, t), rtol=1e-8)
    np.testing.assert_allclose(tr.forced_analytic(vf.u0, vf.p, t0, t0)[0], vf.u0, rtol=1e-15)


@pytest.mark.parametrize("kind", ["EK0", "EK1"])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_fixed_grid_orders(kind, q):
    vf = tr.forced()
    t0, t1 = vf.tspan
    errs = []
    for dt in DTS:
        sol = orc.solve(vf, orc.Alg(kind, q, "dynamic", False), tspan=vf.tspan, dt=dt)
        errs.append(float(np.mean(np.abs(sol.u[-1] - tr.forced_analytic(vf.u0, vf.p, t0, t1)[0]))))
    order = float(np.mean(tr.convergence_orders(errs, DTS)))
    print(kind, q, errs, order)
    assert abs(order - (q + 1)) < 0.2, (order, errs)


def test_adaptive_solve_ends_successfully():
    vf = tr.forced()
    sol = orc.solve(vf, orc.EK1(order=3, smooth=False), tspan=vf.tspan, adaptive=True, abstol=1e-6, reltol=1e-4, dt=1e-2)
    assert sol.retcode == "Success" and len(sol.t) == 52
    err = np.abs(sol.u[-1] - tr.forced_analytic(vf.u0, vf.p, vf.tspan[0], vf.tspan[1])[0]).max()
    assert err < 1e-3
