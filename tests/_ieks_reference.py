"""numpy restatement of the iterated extended Kalman smoother, `IEKS` + `solve_ieks` (src/ieks.jl:2-61), built from the
oracle's pieces.

One iteration is a complete fixed-grid solve -- filter, postamble (the :fixed / :fixedMAP rescale), smoother -- whose EK1
step evaluates the Jacobian at the linearisation point instead of at the prediction (src/perform_step.jl:111-125):
`J = f.jac(linearize_at(tnew).mu)`, `H = (E1 - J E0) PI`, while the residual keeps `f(u_pred)`.  On the previous
iteration's grid `linearize_at(tnew).mu` is exactly the u part of its smoothed mean at that save.  `solve_ieks` starts from
`linearize_at = nothing` (the first iteration is EK1) and has no stopping criterion.

The step is the oracle's own (`orc.solve`) run on a copy of the vector field whose `jac` ignores its argument and returns
the Jacobian at the linearisation point of the step's new time; everything else is untouched.
"""
import dataclasses

import numpy as np

import odefilter_oracle as orc


def linearized_field(vf: orc.VectorField, grid, lin) -> orc.VectorField:
    """`vf` with the Jacobian of the step ending at grid[k] evaluated at lin[k] (lin: [n_t, d]); f is unchanged."""
    grid = np.asarray(grid, float)
    lin = np.asarray(lin, float)

    def jac(u, p, t):
        k = int(np.argmin(np.abs(grid - t)))  # measure! is called at tnew = t + dt, a grid point up to rounding
        return vf.jac(lin[k], p, t)

    return dataclasses.replace(vf, jac=jac)


def solve_once(vf: orc.VectorField, order: int, diffusionmodel: str, grid, *, u0=None, p=None, linearize_at=None) -> orc.Solution:
    """`solve(prob, IEKS(order, diffusionmodel, linearize_at); tgrid=grid)`: `linearize_at` is None (EK1) or the
    linearisation points [n_t, d] on `grid`."""
    grid = np.asarray(grid, float)
    field = vf if linearize_at is None else linearized_field(vf, grid, linearize_at)
    return orc.solve(field, orc.EK1(order=order, diffusionmodel=diffusionmodel, smooth=True), u0=u0, p=p,
                     tspan=(grid[0], grid[-1]), tgrid=grid)


def solve_ieks(vf: orc.VectorField, order: int, diffusionmodel: str, grid, iterations: int = 10, *, u0=None, p=None,
               history: bool = False):
    """src/ieks.jl:52-61: `iterations` solves, each linearised at the previous one's smoothed u.  Returns the last
    solution, or with `history` the list of all of them."""
    sols, lin = [], None
    for _ in range(iterations):
        sol = solve_once(vf, order, diffusionmodel, grid, u0=u0, p=p, linearize_at=lin)
        lin = sol.u  # the smoothed u at every save: linearize_at(t).mu on this grid
        sols.append(sol)
    return sols if history else sols[-1]
