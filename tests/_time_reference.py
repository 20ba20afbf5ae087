"""Reference for time-dependent vector fields f(u, p, t), built from the oracle's pieces.

The oracle's `perform_step` / `measure` already hand the step's new time to `vf.f` and `vf.jac` (src/perform_step.jl:106,117).
Only its `get_derivatives` -- the Taylor-mode initialisation -- hands the field a plain `t0`, which is the reference's own limit
(src/state_initialization.jl:20-22 asserts that f does not depend on t).  `time_field` wraps a field so that, whenever `u` holds
`orc.Jet`s and `t` is a float, `t` becomes the jet [t, 1, 0, ...] of the same length: the recursion coef[k+1] = f(jets)_k / (k+1)
then yields the total derivatives (u'' = f_u f + f_t, ...), and `orc.solve` (and the IEKS / MV restatements on top of it) need no
change.
"""
import dataclasses
import math

import numpy as np

import odefilter_oracle as orc

RHS_FORCED = 7  # ODEF_RHS_FORCED (include/odefilter.h)


def time_field(vf: orc.VectorField) -> orc.VectorField:
    """`vf` whose `f` sees t as a Taylor jet in the initialisation (jets in u, float t); the step is untouched."""
    f = vf.f

    def f_jet(u, p, t):
        if len(u) and isinstance(u[0], orc.Jet) and not isinstance(t, orc.Jet):
            c = np.zeros(len(u[0].c))
            c[0] = t
            c[1] = 1.0
            t = orc.Jet(c)
        return f(u, p, t)

    return dataclasses.replace(vf, f=f_jet)


def _forced_f(u, p, t):
    return [p[0] * u[0] + p[1] * t, p[2] * t * u[1]]


def _forced_jac(u, p, t):
    return np.array([[p[0], 0.0], [0.0, p[2] * t]])


def forced() -> orc.VectorField:
    """u0' = p0 u0 + p1 t (t enters f),  u1' = p2 t u1 (t enters the Jacobian); the non-zero t0 is on purpose."""
    return time_field(orc.VectorField("forced", RHS_FORCED, 2, 3, _forced_f, _forced_jac, np.array([0.5, 1.0]),
                                      np.array([-0.7, 1.3, 0.9]), (0.25, 2.25)))


def forced_analytic(u0, p, t0, t):
    """The closed-form solution of `forced` at the absolute times t ([n] -> [n, 2])."""
    u0 = np.asarray(u0, float)
    t = np.atleast_1d(np.asarray(t, float))
    a, b, c = p
    k = b / (a * a)
    return np.stack([(u0[0] + b * t0 / a + k) * np.exp(a * (t - t0)) - b * t / a - k, u0[1] * np.exp(0.5 * c * (t * t - t0 * t0))], axis=-1)


def forced_derivatives(u0, p, t0):
    """u', u'', u''' of `forced` at t0, written out by hand."""
    a, b, c = p
    x, y = u0
    x1 = a * x + b * t0
    x2 = a * x1 + b
    x3 = a * x2
    y1 = c * t0 * y
    y2 = c * y + c * t0 * y1
    y3 = 2.0 * c * y1 + c * t0 * y2
    return [np.array([x1, y1]), np.array([x2, y2]), np.array([x3, y3])]


def _l96t_f(u, p, t):
    n = len(u)
    return [(u[(i + 1) % n] - u[(i - 2) % n]) * u[(i - 1) % n] - u[i] + (p[0] + p[1] * t) for i in range(n)]


def lorenz96_forced(n: int = 5) -> orc.VectorField:
    """Lorenz-96 with n variables and the forcing F + a t, p = (F, a): a time-dependent field no compiled-in kernel covers."""
    base = orc.vector_field("lorenz96")
    u0 = 2.0 + np.array([0.1 * ((3 * i) % 5 - 2) for i in range(n)])
    return time_field(orc.VectorField("lorenz96_forced", -1, n, 2, _l96t_f, lambda u, p, t: base.jac(u, p, t), u0,
                                      np.array([4.0, 1.5]), (0.5, 1.0)))


def convergence_orders(errs, dts):
    """Observed orders log(e_k / e_{k+1}) / log(dt_k / dt_{k+1})."""
    return [math.log(errs[k] / errs[k + 1]) / math.log(dts[k] / dts[k + 1]) for k in range(len(errs) - 1)]
