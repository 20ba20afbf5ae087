"""The numpy restatement of the MV diffusion models (tests/_mv_reference.py) anchored to the oracle through two exact
identities of EK0 (CPU only):

- d = 1: a diagonal diffusion of one component is the scalar one, so :dynamicMV is :dynamic and :fixedMV is :fixed.
- a field whose components do not interact (u_i' = p_i u_i) separates under EK0 into d independent d = 1 problems on a
  fixed grid: H = E1 P^-1, A = At (x) I and Q = Qt (x) I act component by component, the diagonal diffusion keeps them
  apart, and S is diagonal -- so the MV solve is d scalar solves side by side, its log-likelihood their sum, and every
  cross-component covariance exactly zero.  (Adaptive steps couple the components through the error norm.)
"""
import numpy as np
import pytest

import _mv_reference as mvr
import odefilter_oracle as orc

SCALAR = {"dynamicMV": "dynamic", "fixedMV": "fixed"}


def logistic():
    """The reference's logistic problem u' = p u (1 - u) (test/specific_problems.jl:62), d = 1."""
    f = lambda u, p, t: [p[0] * u[0] * (1.0 - u[0])]  # noqa: E731
    jac = lambda u, p, t: np.array([[p[0] * (1.0 - 2.0 * u[0])]])  # noqa: E731
    return orc.VectorField("logistic", -1, 1, 1, f, jac, np.array([1e-1]), np.array([3.0]), (0.0, 1.0))


def linear1(u0, p):
    return orc.VectorField("linear1", -1, 1, 1, orc._lin_f, orc._lin_jac, np.array([u0]), np.array([p]), (0.0, 1.0))


def _close(a, b, rtol=1e-9, atol=0.0):
    """Rounding-level agreement: the two sides take different (exact-arithmetic equal) paths, and the higher derivatives
    and covariances amplify a rounding difference (tests/_parity.py), so the bar is relative to the array's magnitude."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.nanmax(np.abs(b)) if b.size else 0.0
    assert np.nanmax(np.abs(a - b), initial=0.0) <= rtol * scale + atol, (np.nanmax(np.abs(a - b)), scale)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("model", ["dynamicMV", "fixedMV"])
def test_d1_equals_scalar_model(model, adaptive):
    vf = logistic()
    kw = dict(adaptive=True, dt=1e-2, abstol=1e-7, reltol=1e-5) if adaptive else dict(adaptive=False, dt=2.0**-5)
    mv = mvr.solve(vf, model, 3, tspan=(0.0, 1.0), **kw)
    ref = orc.solve(vf, orc.EK0(order=3, diffusionmodel=SCALAR[model]), tspan=(0.0, 1.0), **kw)
    assert (mv.naccept, mv.nreject) == (ref.naccept, ref.nreject)
    if adaptive:
        assert mv.nreject > 0 or mv.naccept > 10
    _close(np.asarray(mv.t), np.asarray(ref.t))
    _close(mv.means(smoothed=False), ref.means(smoothed=False))
    _close(mv.covs(smoothed=False), ref.covs(smoothed=False))
    _close(mv.means(smoothed=True), ref.means(smoothed=True))
    _close(mv.covs(smoothed=True), ref.covs(smoothed=True))
    _close(np.array(mv.diffusions)[:, 0], np.array(ref.diffusions))
    if model == "fixedMV":
        assert np.isnan(mv.log_likelihood) and np.isnan(ref.log_likelihood)
    else:
        _close(mv.log_likelihood, ref.log_likelihood)


@pytest.mark.parametrize("model", ["dynamicMV", "fixedMV"])
def test_decoupled_field_is_d_scalar_solves(model):
    vf = orc.vector_field("linear")
    q, d, dt, tspan = 2, vf.d, 2.0**-4, (0.0, 1.0)
    D = d * (q + 1)
    mv = mvr.solve(vf, model, q, tspan=tspan, dt=dt)
    m_f, c_f = mv.means(smoothed=False), mv.covs(smoothed=False)
    m_s, c_s = mv.means(smoothed=True), mv.covs(smoothed=True)
    diffs = np.array(mv.diffusions)
    ll = 0.0
    for a in range(d):
        one = orc.solve(linear1(vf.u0[a], vf.p[a]), orc.EK0(order=q, diffusionmodel=SCALAR[model]), tspan=tspan, dt=dt)
        idx = np.arange(q + 1) * d + a
        _close(m_f[:, idx], one.means(smoothed=False))
        _close(m_s[:, idx], one.means(smoothed=True))
        _close(c_f[:, idx][:, :, idx], one.covs(smoothed=False))
        _close(c_s[:, idx][:, :, idx], one.covs(smoothed=True))
        _close(diffs[:, a], np.array(one.diffusions))
        ll += one.log_likelihood
    comp = np.arange(D) % d
    cross = comp[:, None] != comp[None, :]
    assert np.all(c_f[:, cross] == 0.0) and np.all(c_s[:, cross] == 0.0)
    if model == "fixedMV":
        assert np.isnan(mv.log_likelihood)
    else:
        _close(mv.log_likelihood, ll)


def test_dense_output_and_sampling_d1():
    """The MV dense output and sampler at d = 1 against the oracle's scalar ones (same noise stream, same square root)."""
    vf = logistic()
    mv = mvr.solve(vf, "fixedMV", 2, tspan=(0.0, 0.5), dt=2.0**-4)
    ref = orc.solve(vf, orc.EK0(order=2, diffusionmodel="fixed"), tspan=(0.0, 0.5), dt=2.0**-4)
    consts = orc.make_consts(1, 2)
    for tv in (0.03, 0.25, 0.49):
        for sm in (False, True):
            a, b = mvr.dense_output(mv, consts, tv, sm), orc.dense_output(ref, consts, tv, sm)
            _close(a.mu, b.mu)
            _close(a.cov(), b.cov())
    s_mv = mvr.sample_states(mv, consts, 2, seed=7)
    s_ref = orc.sample_states(ref, consts, 2, seed=7, sqrt="cholesky")
    _close(s_mv, s_ref)
