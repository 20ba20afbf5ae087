"""The numpy restatement of IEKS / solve_ieks (tests/_ieks_reference.py) checked against the oracle and against what the
iteration must do (CPU only):

- one iteration is the oracle's EK1 solve and smooth, bit for bit;
- on a linear field J does not depend on the point, so every iteration is that EK1 solve;
- the reference's own IEKS check (test/ieks.jl: FitzHugh-Nagumo, IEKS(order=4, diffusionmodel=:fixed)) on a fixed grid:
  the iterates converge, the change between successive smoothed iterates shrinks from iteration 1 to 6;
- a solve seeded with linearize_at = the EK1 smoothed solution is iteration 2.
"""
import numpy as np
import pytest

import _ieks_reference as ier
import odefilter_oracle as orc


def fhn_problem():
    """examples/fitzhughnagumo_animation.jl:13-15: u0 = [-1, 1], tspan = (0, 20), p = (0.2, 0.2, 3.0)."""
    vf = orc.vector_field("fhn")
    return vf, np.array([-1.0, 1.0]), np.array([0.2, 0.2, 3.0]), (0.0, 20.0)


def _same(a, b):
    np.testing.assert_array_equal(np.asarray(a.means(smoothed=True)), np.asarray(b.means(smoothed=True)))
    np.testing.assert_array_equal(np.asarray(a.covs(smoothed=True)), np.asarray(b.covs(smoothed=True)))
    np.testing.assert_array_equal(np.asarray(a.means(smoothed=False)), np.asarray(b.means(smoothed=False)))
    assert a.diffusions == b.diffusions and (a.log_likelihood == b.log_likelihood or
                                              (np.isnan(a.log_likelihood) and np.isnan(b.log_likelihood)))


@pytest.mark.parametrize("rhs,order,model,dt", [("lorenz63", 3, "dynamic", 2.0**-8), ("fhn", 4, "fixed", 0.05),
                                                ("vanderpol", 5, "fixedMAP", 0.02)])
def test_one_iteration_is_ek1(rhs, order, model, dt):
    vf = orc.vector_field(rhs)
    grid = orc.fixed_time_grid(vf.tspan[0], vf.tspan[1], dt)
    ek1 = orc.solve(vf, orc.EK1(order=order, diffusionmodel=model, smooth=True), tgrid=grid)
    _same(ier.solve_ieks(vf, order, model, grid, iterations=1), ek1)
    assert ek1.njacs == ek1.nf == len(grid) - 1


@pytest.mark.parametrize("model", ["dynamic", "fixed"])
def test_linear_field_every_iteration_is_ek1(model):
    vf = orc.vector_field("linear")
    grid = orc.fixed_time_grid(0.0, 2.0, 0.05)
    ek1 = orc.solve(vf, orc.EK1(order=3, diffusionmodel=model, smooth=True), tgrid=grid)
    for sol in ier.solve_ieks(vf, 3, model, grid, iterations=4, history=True):
        _same(sol, ek1)


def test_fhn_iterates_converge():
    """test/ieks.jl: FitzHugh-Nagumo with IEKS(order=4, diffusionmodel=:fixed), here on the fixed grid dt = 0.1."""
    vf, u0, p, tspan = fhn_problem()
    grid = orc.fixed_time_grid(tspan[0], tspan[1], 0.1)
    sols = ier.solve_ieks(vf, 4, "fixed", grid, iterations=7, u0=u0, p=p, history=True)
    us = [s.u for s in sols]
    assert all(np.all(np.isfinite(u)) for u in us)
    change = [float(np.abs(us[k + 1] - us[k]).max()) for k in range(len(us) - 1)]
    assert change[0] > 1e-6  # the relinearisation does change the solution
    assert all(change[k + 1] < change[k] for k in range(5)), change
    assert change[5] < 1e-3 * change[0], change


def test_seeded_solve_is_iteration_two():
    vf = orc.vector_field("lorenz63")
    grid = orc.fixed_time_grid(0.0, 1.0, 2.0**-7)
    two = ier.solve_ieks(vf, 3, "dynamic", grid, iterations=2)
    ek1 = orc.solve(vf, orc.EK1(order=3, smooth=True), tgrid=grid)
    _same(ier.solve_once(vf, 3, "dynamic", grid, linearize_at=ek1.u), two)
    assert np.abs(two.u - ek1.u).max() > 0.0
